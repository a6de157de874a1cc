"""The row header of the headline row kernels (SweepHead: k_sweep4, k_sweep4q, k_sweep4t).

An extend workgroup takes every address its head loads from, and the plan of the step, from one entry of a table the host
resolves once per call: sixteen entries a chunk, entry (step mod 16), each with the ring slots of rows s_begin + step - 1 and
s_begin + step folded into its pointers.  What that can get wrong, and what the existing parity tests do not pin down:

(i)   the ring phase: calls that start at rows 0, 1, 15 and others mod 16, a call long enough for the ring to wrap twice, calls of
      one and two rows (little more than the flush steps);
(ii)  several chunks in one launch, each with its own entries, one of which runs out of rows early;
(iii) the tree-recording instance (k_sweep4<*, true>, one launch per step);
(iv)  a call that follows single steps of the general kernels: its first step continues from the slot the general kernels left,
      not from a ring slot;
(v)   rows whose segment data is requested (last of all now) although the update loop does not run.

Everything is compared bit for bit: with the oracle (trace, resampling parents, final particles, log-likelihood), in (ii) with the
chunk's own single run."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_run(oracle, key, model, segs, Np, seed):
    """the oracle's uninterrupted run of a case, computed once and shared (read only)"""
    if key not in _ORACLE:
        o = oracle.Oracle(model, Np, seed=seed, max_trace_events=64)
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


def _case(n):
    model = cases.make_model(n=n, E=10, L=1.5e5)
    return model, cases.make_segments(model, seed=20 + n, max_seg_len=4000)


@pytest.mark.parametrize("n,Np", [(4, 1000), (3, 300)])
def test_calls_at_every_ring_phase(oracle, hiplib, n, Np):
    from smcsmc_amd import ParticleFilter
    assert Np % 64 != 0 and Np % 256 != 0              # neither the last wavefront nor the last workgroup is full
    model, segs = _case(n)
    S = len(segs["start"])
    cuts = [0, 1, 15, 22, 67, 69, S]
    assert S > 75, S
    begins, lengths = cuts[:-1], np.diff(cuts)
    assert {b % 16 for b in begins} >= {0, 1, 15} and any(b % 16 not in (0, 1, 15) for b in begins)
    assert lengths.max() > 40 and lengths.min() == 1 and 2 in lengths
    ref = _oracle_run(oracle, (n, Np), model, segs, Np, 9)
    g = ParticleFilter(model, Np, seed=9, max_trace_events=64)
    assert g.run_path() == "SweepSplit"
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.run(a, b)
    g.finish()
    _equals_oracle(ref, g)
    g.close()


def test_chunks_with_their_own_entries(hiplib):
    """Three filters of different seeds and lengths, whose data start at different rows of the set, through run_many in calls that
    start at several ring phases: each equals its own single run.  (One call has one first row for all its chunks: what differs
    between the entries of two chunks is every pointer and the last row.)"""
    from smcsmc_amd import ParticleFilter
    model, segs = _case(4)
    S = len(segs["start"])
    offs, ends = [0, 5, 18], [S, S - 30, 64]

    def new(k):
        sub = {key: np.ascontiguousarray(v[offs[k]:ends[k]]) for key, v in segs.items()}
        f = ParticleFilter(model, 1000, seed=3 + k, max_trace_events=64)
        f.init_prior(sub["start"][0]); f.load_segments(sub)
        return f

    alone = [new(k) for k in range(3)]
    for f in alone:
        f.run(); f.finish()
    many = [new(k) for k in range(3)]
    nmax = max(f.n_segs for f in many)
    assert many[2].n_segs == 46 and many[2].n_segs < many[1].n_segs < many[0].n_segs
    cuts = [0, 15, 17, 33, 46 + 11, nmax]               # the third chunk ends inside the fourth call and sits the fifth out
    for a, b in zip(cuts[:-1], cuts[1:]):
        ParticleFilter.run_many(many, a, b)
    resampling = 0
    for f, g in zip(many, alone):
        f.finish()
        assert f.segments_done() == g.segments_done() == f.n_segs
        tf, tg = f.trace(), g.trace()
        for k in ("T", "ess", "logl"):
            assert (_bits(tf[k]) == _bits(tg[k])).all(), k
        assert (tf["resampled"] == tg["resampled"]).all()
        (sf, pf_), (sg, pg) = f.resample_events(), g.resample_events()
        assert (sf == sg).all() and (pf_ == pg).all()
        resampling += len(sf)
        wf, wg = f.particles(), g.particles()
        for k in wf:
            assert (np.asarray(wf[k]).view(np.uint8) == np.asarray(wg[k]).view(np.uint8)).all(), k
        assert _bits([f.logl()])[0] == _bits([g.logl()])[0]
        cf, cg = f.counts(), g.counts()
        for k in cf:
            assert (_bits(cf[k]) == _bits(cg[k])).all(), k
    assert resampling >= 3
    for f in many + alone:
        f.close()


def test_tree_recording_instance(oracle, hiplib):
    from smcsmc_amd import ParticleFilter
    model = cases.make_model(n=4, E=10, L=6e4)
    segs = cases.make_segments(model, seed=24, max_seg_len=3000)
    g = ParticleFilter(model, 300, seed=4, max_trace_events=0, record_trees=True, log_cap=8192, gen_cap=4096)
    assert g.run_path() == "Sweep"
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(0, 21); g.run(21, g.n_segs); g.finish()
    assert g.trace()["resampled"].sum() >= 3
    part, kind, pos, hgt, desc = g.sample_tree_events()
    o = oracle.Oracle(model, 300, seed=4, max_trace_events=0)
    o.enable_tree_recording()
    o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    opart, okind, opos, ohgt, odesc = o.sample_tree_events()
    assert opart == part and len(okind) == len(kind) and (okind == kind).all() and (odesc == desc).all()
    assert (_bits(opos) == _bits(pos)).all() and (_bits(ohgt) == _bits(hgt)).all()
    assert _bits([o.logl()])[0] == _bits([g.logl()])[0]
    g.close(); o.close()


def test_run_after_single_steps(oracle, hiplib):
    """Five rows by update_segment / count / resample (the general kernels: two state buffers), the rest by run(): the first step of
    that call continues from the buffer the general kernels left, rows 6 onwards from the ring."""
    from smcsmc_amd import ParticleFilter
    model, segs = _case(4)
    ref = _oracle_run(oracle, (4, 1000), model, segs, 1000, 9)
    g = ParticleFilter(model, 1000, seed=9, max_trace_events=64)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    for s in range(5):
        g.update_segment(s); g.count(s); g.resample(s)
    g.run(5, g.n_segs)
    g.finish()
    _equals_oracle(ref, g)
    g.close()


def test_second_launches_one_by_one(oracle, hiplib):
    """The ledger and count launches of one chunk follow its extend launches in batches of four steps behind one completion signal, as
    those of several chunks always did; bits 16-19 of pf_params.debug = 1 keep the earlier arrangement, one by one: the same bits, in calls
    of 41 rows (a call ends inside a batch)."""
    from smcsmc_amd import ParticleFilter
    model, segs = _case(4)
    ref = _oracle_run(oracle, (4, 1000), model, segs, 1000, 9)
    for debug in (0, 1 << 16):
        g = ParticleFilter(model, 1000, seed=9, max_trace_events=64, debug=debug)
        g.init_prior(segs["start"][0]); g.load_segments(segs)
        for a in range(0, g.n_segs, 41):
            g.run(a, min(g.n_segs, a + 41))
        g.finish()
        _equals_oracle(ref, g)
        g.close()


def test_rows_whose_loop_does_not_run(oracle, hiplib):
    """the construction of test_gpu_row_chain: rows in which every sample is missing, and a last row that ends past the sequence"""
    from smcsmc_amd import ParticleFilter
    n, Np, L = 4, 1000, 1.2e5
    model = cases.make_model(n=n, E=10, L=L)
    segs = cases.make_segments(model, seed=31, max_seg_len=3000, missing_block=(3.0e4, 5.0e4, list(range(n))))
    al = segs["alleles"]
    part = (segs["start"] >= 7.0e4) & (segs["start"] < 8.0e4)
    al[part, 0] = -1
    assert int((al == -1).all(axis=1).sum()) >= 3
    segs["length"][-1] += 7000.0
    al[-1, :] = -1
    assert segs["start"][-1] + segs["length"][-1] > L
    ref = _oracle_run(oracle, "no data", model, segs, Np, 4)
    assert len(ref["trace"]["T"]) == len(segs["start"])
    g = ParticleFilter(model, Np, seed=4, max_trace_events=64, local_recomb=True)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(); g.finish()
    _equals_oracle(ref, g, min_resampling=1)
    g.close()
    # a sequence that ends inside an earlier row: the rows behind it are not run
    short = dict(model, loci_length=9.05e4)
    ref = _oracle_run(oracle, "short", short, segs, Np, 4)
    assert len(ref["trace"]["T"]) < len(segs["start"])
    g = ParticleFilter(short, Np, seed=4, max_trace_events=64)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(); g.finish()
    _equals_oracle(ref, g, min_resampling=0)
    g.close()
