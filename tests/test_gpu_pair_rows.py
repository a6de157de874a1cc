"""The paired form of the headline row kernel (k_sweep4p, csrc/pf_pair.h): an extend workgroup owns 128 particles, two tree wavefronts
run the genealogy's chain and two weight wavefronts beside them apply the no-mutation factors (handed over through a ring of eight entries a
lane in LDS), do the old slot's part of a resampling row and the row's scans.  It runs where every extend workgroup of a call can have a
compute unit of its own (chunks * ceil(Np / 128) <= compute units) and no handle has vb_coal: row_form() says which form ran, after every call.

Everything is bit for bit with the oracle by the conventions of test_gpu_row_head.py (trace, resampling parents, final particles,
log-likelihood), and with the one-wavefront form of the same handle (PF_DEBUG_NO_PAIR).  What the form can get wrong:

(i)   the shapes: a second tree wavefront that is empty (Np = 64) or holds one particle (65), a last workgroup partly filled (129, 300, 1000),
      the instance for four haplotypes and the one for fewer;
(ii)  resampling rows (nearly all, some, none): the split of the parent search, the old slot's records written by the other wavefront;
(iii) the ring: rows with several times its depth in updates (wrap, back-pressure);
(iv)  rows whose loop does not run, flush steps, calls of one and two rows, every ring phase of the row header, a first step that continues
      from the general kernels;
(v)   several chunks in one launch, the rule that chooses the form, and vb_coal handles, which keep the one-wavefront form.

Every case held to the oracle runs in both forms (the `form` fixture: PF_DEBUG_NO_PAIR for the one-wavefront form).

No case waits for a spin to expire."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_run(oracle, key, model, segs, Np, seed, ess_fraction=0.5):
    """the oracle's uninterrupted run of a case, computed once and shared (read only)"""
    if key not in _ORACLE:
        o = oracle.Oracle(model, Np, ess_fraction=ess_fraction, seed=seed, max_trace_events=64)
        o.init_prior(segs["start"][0])
        o.run(o.pack_segments(model, segs))
        _ORACLE[key] = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), logl=o.logl())
        o.close()
    return _ORACLE[key]


def _equals_oracle(ref, g, min_resampling=3):
    to, tg = ref["trace"], g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    (so, po), (sg, pg) = ref["events"], g.resample_events()
    assert len(so) >= min_resampling, "the case hardly resamples: it checks little of the completion of a row"
    assert (so == sg).all() and (po == pg).all()
    ps_o, ps_g = ref["particles"], g.particles()
    assert (ps_o["children"] == ps_g["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(ps_o[k]) == _bits(ps_g[k])).all(), k
    assert _bits([ref["logl"]])[0] == _bits([g.logl()])[0]


def _same_run(f, g, exact_counts=False):
    """two filters of the library: every output equal, bit for bit (the count columns of the two forms: to the last bit, or within the
    suite's 1e-9; of a chunk and its own single run: to the last bit)"""
    tf, tg = f.trace(), g.trace()
    assert f.segments_done() == g.segments_done()
    for k in ("T", "ess", "logl"):
        assert (_bits(tf[k]) == _bits(tg[k])).all(), k
    assert (tf["resampled"] == tg["resampled"]).all()
    (sf, pf_), (sg, pg) = f.resample_events(), g.resample_events()
    assert (sf == sg).all() and (pf_ == pg).all()
    wf, wg = f.particles(), g.particles()
    for k in wf:
        assert (np.asarray(wf[k]).view(np.uint8) == np.asarray(wg[k]).view(np.uint8)).all(), k
    assert _bits([f.logl()])[0] == _bits([g.logl()])[0]
    cf, cg = f.counts(), g.counts()
    for k in cf:
        if exact_counts:
            assert (_bits(cf[k]) == _bits(cg[k])).all(), k
        else:
            np.testing.assert_allclose(cf[k], cg[k], rtol=1e-9, atol=1e-300, err_msg=k)
    return len(sf)


def _case(n):
    model = cases.make_model(n=n, E=10, L=1.5e5)
    return model, cases.make_segments(model, seed=20 + n, max_seg_len=4000)


@pytest.fixture(params=["paired", "single"])
def form(request):
    """every case that is held to the oracle runs in both forms of the row kernel: as the rule chooses, and with PF_DEBUG_NO_PAIR"""
    return request.param


def _run(model, segs, Np, seed, cuts=None, form="paired", expect=None, **kw):
    from smcsmc_amd import ParticleFilter, pf
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=64, debug=pf.DEBUG_NO_PAIR if form == "single" else 0, **kw)
    assert g.run_path() == "SweepSplit"
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    cuts = cuts or [0, g.n_segs]
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run(a, b)
        assert g.row_form() == (expect or form)
    g.finish()
    return g


@pytest.mark.parametrize("Np", [64, 65, 129, 300, 1000])
@pytest.mark.parametrize("n", [4, 3, 2])
def test_shapes(oracle, hiplib, form, n, Np):
    model, segs = _case(n)
    ref = _oracle_run(oracle, ("shape", n, Np), model, segs, Np, 9)
    g = _run(model, segs, Np, 9, form=form)
    _equals_oracle(ref, g)
    g.close()


@pytest.mark.parametrize("Np", [129, 300])
@pytest.mark.parametrize("ess", [0.9, 0.5, 1e-4])
def test_resampling_rates(oracle, hiplib, form, ess, Np):
    model, segs = _case(4)
    ref = _oracle_run(oracle, ("ess", ess, Np), model, segs, Np, 5, ess_fraction=ess)
    rows, resampling = len(ref["trace"]["T"]), int(ref["trace"]["resampled"].sum())
    if ess == 0.9:
        assert resampling > 0.9 * rows, (resampling, rows)          # nearly every row resamples
    if ess == 1e-4:
        assert resampling == 0 and len(ref["events"][0]) == 0
    g = _run(model, segs, Np, 5, ess_fraction=ess, form=form)
    _equals_oracle(ref, g, min_resampling=0 if ess == 1e-4 else 3)
    g.close()


@pytest.mark.parametrize("Np", [129, 300])
def test_ring_wraps(oracle, hiplib, form, Np):
    """Ten times the recombination rate: the oracle makes 4.8 updates per lane and row on average over these 264 rows, and the rows of
    4000 bp take several times the ring's eight entries -- the ring wraps, and a tree lane has to wait for its weight lane."""
    model = cases.make_model(n=4, E=10, L=1.5e5, rho=1e-7)
    segs = cases.make_segments(model, seed=24, max_seg_len=4000)
    assert len(segs["start"]) == 264 and segs["length"].max() == 4000.0
    ref = _oracle_run(oracle, ("wrap", Np), model, segs, Np, 9)
    g = _run(model, segs, Np, 9, form=form)
    _equals_oracle(ref, g)
    g.close()


def test_rows_without_data(oracle, hiplib, form):
    model = cases.make_model(n=4, E=10, L=6e4)
    segs = cases.nodata_segments(model)
    ref = _oracle_run(oracle, "nodata", model, segs, 300, 4)
    g = _run(model, segs, 300, 4, form=form)
    _equals_oracle(ref, g, min_resampling=0)
    g.close()


def test_rows_whose_loop_does_not_run(oracle, hiplib, form):
    """the construction of test_gpu_row_head: rows in which every sample is missing, a last row that ends past the sequence, and a sequence
    that ends inside an earlier row (the two flush steps follow it)"""
    n, Np, L = 4, 300, 1.2e5
    model = cases.make_model(n=n, E=10, L=L)
    segs = cases.make_segments(model, seed=31, max_seg_len=3000, missing_block=(3.0e4, 5.0e4, list(range(n))))
    al = segs["alleles"]
    al[(segs["start"] >= 7.0e4) & (segs["start"] < 8.0e4), 0] = -1
    assert int((al == -1).all(axis=1).sum()) >= 3
    segs["length"][-1] += 7000.0
    al[-1, :] = -1
    assert segs["start"][-1] + segs["length"][-1] > L
    ref = _oracle_run(oracle, "no data rows", model, segs, Np, 4)
    g = _run(model, segs, Np, 4, local_recomb=True, form=form)
    _equals_oracle(ref, g, min_resampling=1)
    g.close()
    short = dict(model, loci_length=9.05e4)
    ref = _oracle_run(oracle, "short", short, segs, Np, 4)
    assert len(ref["trace"]["T"]) < len(segs["start"])
    g = _run(short, segs, Np, 4, form=form)
    _equals_oracle(ref, g, min_resampling=0)
    g.close()


@pytest.mark.parametrize("n,Np", [(4, 1000), (3, 300)])
def test_calls_at_every_ring_phase(oracle, hiplib, form, n, Np):
    """calls that begin at ring phases 0, 1, 15 and another, calls of one and of two rows"""
    model, segs = _case(n)
    S = len(segs["start"])
    cuts = [0, 1, 15, 22, 67, 69, S]
    lengths = np.diff(cuts)
    assert {b % 16 for b in cuts[:-1]} >= {0, 1, 15} and lengths.min() == 1 and 2 in lengths and lengths.max() > 40
    ref = _oracle_run(oracle, ("shape", n, Np), model, segs, Np, 9)
    g = _run(model, segs, Np, 9, cuts=cuts, form=form)
    _equals_oracle(ref, g)
    g.close()


def test_run_after_single_steps(oracle, hiplib, form):
    """five rows by the general kernels, the rest by run(): the first step of that call continues from the buffer they left"""
    from smcsmc_amd import ParticleFilter, pf
    model, segs = _case(4)
    ref = _oracle_run(oracle, ("shape", 4, 1000), model, segs, 1000, 9)
    g = ParticleFilter(model, 1000, seed=9, max_trace_events=64, debug=pf.DEBUG_NO_PAIR if form == "single" else 0)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    for s in range(5):
        g.update_segment(s); g.count(s); g.resample(s)
    g.run(5, g.n_segs)
    assert g.row_form() == form
    g.finish()
    _equals_oracle(ref, g)
    g.close()


@pytest.mark.parametrize("n,Np,rho", [(4, 1000, 1e-8), (4, 129, 1e-7), (3, 65, 1e-8), (2, 300, 1e-8)])
def test_both_forms(hiplib, n, Np, rho):
    """the same handle with and without PF_DEBUG_NO_PAIR, in calls that end inside a batch of second launches"""
    model = cases.make_model(n=n, E=10, L=1.5e5, rho=rho)
    segs = cases.make_segments(model, seed=24, max_seg_len=4000)
    cuts = list(range(0, len(segs["start"]), 41)) + [len(segs["start"])]
    a = _run(model, segs, Np, 7, cuts=cuts, local_recomb=True)
    b = _run(model, segs, Np, 7, cuts=cuts, local_recomb=True, form="single")
    assert _same_run(a, b) >= 3
    a.close(); b.close()


def test_two_chunks(hiplib):
    """two chunks through run_many run the paired form, and each equals its own single run"""
    from smcsmc_amd import ParticleFilter
    model, segs = _case(4)
    S = len(segs["start"])
    offs, ends = [0, 18], [S, S - 30]

    def new(k):
        sub = {key: np.ascontiguousarray(v[offs[k]:ends[k]]) for key, v in segs.items()}
        f = ParticleFilter(model, 1000, seed=3 + k, max_trace_events=64)
        f.init_prior(sub["start"][0]); f.load_segments(sub)
        return f

    alone = [new(k) for k in range(2)]
    for f in alone:
        f.run(); f.finish()
    many = [new(k) for k in range(2)]
    nmax = max(f.n_segs for f in many)
    for a, b in zip([0, 15, 17, 33], [15, 17, 33, nmax]):
        ParticleFilter.run_many(many, a, b)
        assert [f.row_form() for f in many] == ["paired", "paired"]
    resampling = 0
    for f, g in zip(many, alone):
        f.finish()
        assert f.segments_done() == f.n_segs
        resampling += _same_run(f, g, exact_counts=True)
    assert resampling >= 3
    for f in many + alone:
        f.close()


def test_vb_coal_keeps_the_one_wavefront_form(oracle, hiplib):
    """With the variational-Bayes correction the update loop multiplies the weights by a factor of its own (particle.cpp:266-272), which the
    ring of the pairs does not carry: such a handle keeps the one-wavefront form where the rule would otherwise choose the paired one, alone
    and in a call it shares with plain handles (the call then runs one form for all), and equals the oracle."""
    from smcsmc_amd import ParticleFilter
    E, Np = 10, 300
    plain, segs = _case(4)
    vb = dict(plain, vb_coal_counts=np.random.default_rng(5).uniform(0.5, 40.0, (E, 1)))
    ref_vb = _oracle_run(oracle, "vb", vb, segs, Np, 6)
    ref_plain = _oracle_run(oracle, "vb: plain", plain, segs, Np, 6)
    assert ref_vb["logl"] != ref_plain["logl"]                      # the correction changes the weights
    g = _run(vb, segs, Np, 6, cuts=[0, 40, len(segs["start"])], expect="single")
    _equals_oracle(ref_vb, g)
    g.close()

    def new(model):
        f = ParticleFilter(model, Np, seed=6, max_trace_events=64)
        f.init_prior(segs["start"][0]); f.load_segments(segs)
        return f
    pair = [new(plain), new(vb)]
    assert ParticleFilter.can_run_many(pair)
    for a, b in ((0, 40), (40, pair[0].n_segs)):
        ParticleFilter.run_many(pair, a, b)
        assert [f.row_form() for f in pair] == ["single", "single"]
    for f, ref in zip(pair, (ref_plain, ref_vb)):
        f.finish()
        _equals_oracle(ref, f)
    for f in pair:
        f.close()
    # (the plain handle on its own takes the paired form: test_shapes)


def test_form_by_compute_units(hiplib):
    """The rule is host arithmetic: chunks * ceil(Np / 128) <= compute units.  Chunks of 1000 particles take eight extend workgroups each: as many
    as just fit run the paired form, one more and the call keeps the one-wavefront form; a few rows are enough to see which ran."""
    from smcsmc_amd import ParticleFilter
    cus = hiplib.pf_device_cus(0)
    assert cus >= 16
    model = cases.make_model(n=4, E=4, L=2e4)
    segs = cases.make_segments(model, seed=3, max_seg_len=2000)
    fit = cus // 8
    fs = [ParticleFilter(model, 1000, seed=1 + k, max_trace_events=0, log_cap=256, gen_cap=64) for k in range(fit + 1)]
    for f in fs:
        f.init_prior(segs["start"][0]); f.load_segments(segs)
    ParticleFilter.run_many(fs[:fit], 0, 3)
    assert {f.row_form() for f in fs[:fit]} == {"paired"} and fs[fit].row_form() is None
    ParticleFilter.run_many(fs, 3, 6)
    assert {f.row_form() for f in fs} == {"single"}
    for f in fs:
        f.finish(); f.close()
