"""Chunks of 9 to 16 haplotypes in lockstep (pf_run_many on the row pipeline with the tree in LDS: one k_sweep_xl launch and one
k_sweep_blc<16, 1, *> launch per row for all chunks).  Every chunk must be bit-identical to its own pf_run -- which stays on the
general kernels (k_extend, k_decide, k_resample, k_count<16, 1>, k_ledger) -- and to the oracle, whatever the calls are cut into,
whoever leads, and whatever runs on a handle in between; groups the launches cannot serve are refused."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError

pytestmark = pytest.mark.gpu

FRACTIONS = (0.5, 0.7, 0.85, 1.0)
GROUPS = [(16, 640, "plain"), (12, 500, "focused"), (9, 200, "guide")]
PLAIN, FOCUSED, GUIDE = GROUPS
CALL = 29
FORCE_LDS = 1        # PF_DEBUG_FORCE_LDS


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _chunks(n, kind):
    """four chunks of one model: lengths 0.5, 0.7, 0.85 and 1.0 x 1.2e5, each with its own data"""
    out = []
    for k, frac in enumerate(FRACTIONS):
        base = cases.make_model(n=n, E=8, L=1.2e5 * frac)
        segs = cases.make_segments(base, seed=70 + 10 * n + 3 * k, max_seg_len=4000)
        model = base
        if kind == "focused":
            model = dict(base, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(8, 2500.0), delay_type=0)
        elif kind == "guide":
            model = dict(base, guide=cases.guide(base, 9, 2.5, n + k), application_delays=np.full(8, 3000.0))
        out.append((model, segs))
    return out


def _new(model, segs, Np, seed, **kw):
    f = ParticleFilter(model, Np, seed=seed, local_recomb=True, **kw)
    f.init_prior(0.0); f.load_segments(segs)
    return f


def _snap(f):
    """everything the comparisons read, so that the filter itself can go"""
    s, p = f.resample_events()
    return dict(logl=f.logl(), trace=f.trace(), rs=(s, p), counts=f.counts(), particles=f.particles(),
                lmap=f.local_recomb(), done=f.segments_done(), rows=f.n_segs)


@functools.lru_cache(maxsize=None)
def _alone(n, Np, kind, count_wgs=0):
    """pf_run of every chunk on its own (the general kernels), computed once per shape and left unchanged"""
    out = []
    for k, (m, sg) in enumerate(_chunks(n, kind)):
        f = _new(m, sg, Np, 3 + k, count_wgs=count_wgs)
        f.run(); f.finish()
        out.append(_snap(f))
        f.close()
    return out


def _group(n, Np, kind, count_wgs=0):
    return [_new(m, sg, Np, 3 + k, count_wgs=count_wgs) for k, (m, sg) in enumerate(_chunks(n, kind))]


def _lockstep(many, call):
    nmax = max(f.n_segs for f in many)
    for s0 in range(0, nmax, call):                         # chunks that are done sit the later calls out
        ParticleFilter.run_many(many, s0, min(nmax, s0 + call))
    for f in many:
        f.finish()


def _same_lmap(a, b):
    """the local recombination map is built with atomics (same terms, any order): the rule of test_gpu_sweep_structured.py"""
    for k in a:
        ref = np.asarray(b[k], dtype=np.float64)
        np.testing.assert_allclose(a[k], ref, rtol=1e-9, atol=1e-12 * max(1e-300, float(np.abs(ref).max())), err_msg=k)


def _same(a, b, counts_rtol=None):
    """a, b: snapshots.  Log-likelihood, traces, resampling, counts and particles bit for bit (counts_rtol: the counts to that
    tolerance instead); the local recombination map by _same_lmap"""
    assert a["done"] == b["done"]
    assert _bits(a["logl"]) == _bits(b["logl"])
    for k in ("T", "ess", "logl"):
        assert (_bits(a["trace"][k]) == _bits(b["trace"][k])).all(), k
    assert (a["trace"]["resampled"] == b["trace"]["resampled"]).all()
    assert (a["rs"][0] == b["rs"][0]).all() and (a["rs"][1] == b["rs"][1]).all()
    for k in a["counts"]:
        if counts_rtol is None:
            assert (_bits(a["counts"][k]) == _bits(b["counts"][k])).all(), k
        else:
            np.testing.assert_allclose(a["counts"][k], b["counts"][k], rtol=counts_rtol, atol=1e-300, err_msg=k)
    for k in a["particles"]:
        assert (np.asarray(a["particles"][k]).view(np.uint8) == np.asarray(b["particles"][k]).view(np.uint8)).all(), k
    _same_lmap(a["lmap"], b["lmap"])


def _all_same(many, alone):
    for f, g in zip(many, alone):
        _same(_snap(f), g)


@pytest.mark.parametrize("n,Np,kind", GROUPS)
def test_chunks_of_9_to_16_haplotypes_in_lockstep_equal_their_own_runs(hiplib, n, Np, kind):
    """Four chunks with their own data, lengths and seeds through pf_run_many in calls of 29 rows (a finished chunk sits the later
    calls out, every call re-seeds the window state): each equals its pf_run on the general kernels.  Np = 500 and 200 leave the
    last 256-lane workgroup partly filled, 640 is two and a half; plain, focused sampling with delays, a guide."""
    alone = _alone(n, Np, kind)
    many = _group(n, Np, kind)
    assert ParticleFilter.can_run_many(many)
    assert len({f.n_segs for f in many}) == len(many)                       # the chunks end at different rows
    assert min(f.n_segs for f in many) >= 40                                # the sixteen-slot rings wrap, the every-eighth-step wait is reached
    _lockstep(many, CALL)
    for f in many:
        assert int(f.trace()["resampled"].sum()) >= 3
    _all_same(many, alone)


@pytest.mark.parametrize("group,which", [(PLAIN, 1), (FOCUSED, 2)], ids=["16-plain-chunk1", "12-focused-chunk2"])
def test_a_lockstep_chunk_equals_the_oracle(oracle, hiplib, group, which):
    """Log-likelihood, resampling parents and final trees bit for bit the oracle's; the counts to 1e-9 (sums in another order); the
    per-sample rows of the local recombination map by the rule of the atomics."""
    n, Np, kind = group
    many = _group(n, Np, kind)
    _lockstep(many, CALL)
    model, segs = _chunks(n, kind)[which]
    g = many[which]
    o = oracle.Oracle(model, Np, seed=3 + which)
    o.enable_local_recomb()
    o.init_prior(0.0); o.run(o.pack_segments(model, segs))
    assert _bits(g.logl()) == _bits(o.logl())
    so, po_ = o.resample_events(); sg, pg_ = g.resample_events()
    assert len(so) >= 3 and (so == sg).all() and (po_ == pg_).all()
    po, pg = o.particles(), g.particles()
    assert (po["children"] == pg["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(po[k]) == _bits(pg[k])).all(), k
    co, cg = o.counts(), g.counts()
    for k in ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight"):
        np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-300, err_msg=k)
    assert cg["resample_count"] == co["resample_count"]
    lo, lg = o.local_recomb(model["loci_length"]), g.local_recomb()
    ref = np.asarray(lo["counts"][:n], dtype=np.float64)
    assert ref.sum() > 0
    np.testing.assert_allclose(lg["counts"][:n], ref, rtol=1e-9, atol=1e-12 * float(np.abs(ref).max()))


def test_a_guide_alone_counts_its_delayed_factors(oracle, hiplib):
    """A guide without height bands delays its factors as well (application_delays): the span over which particles carried
    pending factors (update_delayed_weight_count, count.cpp:395-397) is the oracle's on the general kernels, which test 1 then
    holds the lockstep run to bit for bit.  The oracle adds the width of a row's window once per such particle, the kernels
    multiply it by their number: every term is positive and differs by at most Np roundings, so 1e-12 (the bound of
    test_gpu_parity.py for focused sampling) is far above (Np + rows) * 2^-53 = 6e-14."""
    n, Np, kind = GUIDE
    model, segs = _chunks(n, kind)[0]
    o = oracle.Oracle(model, Np, seed=3)
    o.init_prior(0.0); o.run(o.pack_segments(model, segs))
    co, cg = o.counts(), _alone(n, Np, kind)[0]["counts"]
    assert co["delayed_count"] > 0
    assert cg["delayed_count"] == pytest.approx(co["delayed_count"], rel=1e-12)
    np.testing.assert_allclose(cg["delayed_opp"], co["delayed_opp"], rtol=1e-12)


def test_call_cuts_and_leader_do_not_matter(hiplib):
    """The n = 16 group in one call, in calls of 7 rows, and with the handle order reversed (another leader, another blockIdx.y for
    every chunk): the same bits, those of the runs alone."""
    n, Np, kind = PLAIN
    alone = _alone(n, Np, kind)
    one = _group(n, Np, kind)
    ParticleFilter.run_many(one)
    for f in one:
        f.finish()
    cut = _group(n, Np, kind)
    _lockstep(cut, 7)
    rev = _group(n, Np, kind)
    _lockstep(rev[::-1], CALL)
    for f, g, r, ref in zip(one, cut, rev, alone):
        _same(_snap(f), _snap(g))
        _same(_snap(f), _snap(r))
        _same(_snap(f), ref)


def test_pf_run_and_step_api_mix_with_lockstep(hiplib):
    """The n = 9 group: 60 rows in lockstep, then 11 rows of chunk 2 by pf_run and of chunk 3 by single steps (update_segment /
    count / resample) on their own handles and streams while the other two take theirs in lockstep, then the rest together: the
    uninterrupted run of every chunk."""
    n, Np, kind = GUIDE
    alone = _alone(n, Np, kind)
    many = _group(n, Np, kind)
    nmax = max(f.n_segs for f in many)
    assert min(f.n_segs for f in many) > 71
    ParticleFilter.run_many(many, 0, 60)
    many[2].run(60, 71)
    for s in range(60, 71):
        many[3].update_segment(s); many[3].count(s); many[3].resample(s)
    ParticleFilter.run_many(many[:2], 60, 71)
    ParticleFilter.run_many(many, 71, nmax)
    for f in many:
        f.finish()
    _all_same(many, alone)


def test_count_wgs_changes_only_the_grouping(hiplib):
    """count_wgs = 2 on the n = 12 group: the lockstep run equals each chunk's own pf_run with count_wgs = 2 bit for bit, and the
    default width to 1e-9 (the sums of a column are grouped by workgroup)."""
    n, Np, kind = FOCUSED
    alone2 = _alone(n, Np, kind, 2)
    many = _group(n, Np, kind, 2)
    assert ParticleFilter.can_run_many(many)
    _lockstep(many, CALL)
    _all_same(many, alone2)
    for f, ref in zip(many, _alone(n, Np, kind)):
        _same(_snap(f), ref, counts_rtol=1e-9)


@pytest.mark.parametrize("count_wgs", [2, 3])
def test_count_wgs_narrower_than_the_particle_blocks_groups_both_paths_alike(hiplib, count_wgs):
    """The n = 16 group has three blocks of 256 particles (Np = 640) and lags from 3 007 bases up.  count_wgs = 2: every column
    two workgroups where the default has three.  count_wgs = 3: the taper (pf_create: ceil(3 * 2500 / lag), at least 2) gives the
    oldest epoch's column three and the others two, what bin/smcsmc sets with six or more chunks.  The chunk's own pf_run and
    pf_finish (k_count_cw on the general kernels) group as the lockstep run does: bit for bit.  Against the default width the
    counts differ by the grouping alone (1e-9), and they do differ, so the width was applied."""
    n, Np, kind = PLAIN
    widths = [int(np.ceil(count_wgs * min(1.0, 2500.0 / lag))) for lag in _chunks(n, kind)[0][0]["lags"]]
    assert (Np + 255) // 256 == 3 and min(max(2, w) for w in widths) < 3
    alone = _alone(n, Np, kind, count_wgs)
    many = _group(n, Np, kind, count_wgs)
    assert ParticleFilter.can_run_many(many)
    _lockstep(many, CALL)
    _all_same(many, alone)
    regrouped = False
    for a, ref in zip(alone, _alone(n, Np, kind)):
        _same(a, ref, counts_rtol=1e-9)
        regrouped |= any((_bits(a["counts"][k]) != _bits(ref["counts"][k])).any() for k in ("coal_opp", "rec_opp", "coal_count"))
    assert regrouped


def _refused(group):
    assert not ParticleFilter.can_run_many(group)
    with pytest.raises(PfError, match="pf_run_many.*16"):
        ParticleFilter.run_many(group)


def test_groups_the_launches_cannot_serve_are_refused(hiplib):
    def pair(n, seed=2, **kw):
        base = cases.make_model(n=n, E=6, L=4e4)
        segs = cases.make_segments(base, seed=seed, max_seg_len=4000)
        return base, segs, [_new(base, segs, 256, 1, **kw), _new(base, segs, 256, 2, **kw)]
    b16, s16, g16 = pair(16)
    b12, s12, g12 = pair(12)
    b8, s8, g8 = pair(8)
    assert ParticleFilter.can_run_many(g16) and ParticleFilter.can_run_many(g12) and ParticleFilter.can_run_many(g16[:1])
    with pytest.raises(PfError, match="twice"):
        ParticleFilter.run_many([g16[0], g16[0]])
    _refused([g16[0], g12[0]])                                              # another width of the tree columns
    _refused([g12[0], g16[0]])
    _refused([g16[0], g8[0]])                                               # the register tree
    _refused([g8[0], g16[0]])
    _refused([g16[0], _new(b16, s16, 256, 2, debug=FORCE_LDS)])             # a debug switch that selects a path
    _refused([_new(b16, s16, 256, 1, debug=FORCE_LDS), _new(b16, s16, 256, 2, debug=FORCE_LDS)])
    _refused([_new(b12, s12, 256, 1, record_trees=True), _new(b12, s12, 256, 2, record_trees=True)])      # -arg
    _refused([g12[0], _new(b12, s12, 256, 2, record_trees=True)])
    m12 = cases.make_structured(b12, P=2, split_epoch=4, mig=1.5)           # structured models above 8 haplotypes
    _refused([_new(m12, s12, 256, 1), _new(m12, s12, 256, 2)])
    _refused([g12[0], _new(m12, s12, 256, 2)])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binary_chunks_side_by_side_at_12_haplotypes(hiplib, built_binary, tmp_path):
    """bin/smcsmc -chunks 4 on twelve haplotypes: one rank filters its four chunks side by side (pf_run_many on the LDS tree), two
    ranks two each; the .out files are the same bytes (the rule of test_gpu_chunks.py), and every chunk leaves its map."""
    from smcsmc_amd import simulate
    n, L = 12, 240000
    base = cases.make_model(n=n, E=8, L=float(L))
    seg = str(tmp_path / "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(L), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=70 + 10 * n))           # the sites cases.make_segments simulates
    core = ("-N0 10000 -t %g -r %g %d -eN 0 1 -eN 0.01 1 -eN 0.25 1 -eN 1 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", str(n), "-seg", seg, "-Np", "300", "-tmax", "4", "-lag", "30000", "-seed", "5", "-chunks", "4"]

    def run(name, extra):
        r = subprocess.run([built_binary] + core + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-400:])
        return open(tmp_path / (name + ".out")).read(), r.stderr

    one, err1 = run("r1", ["-ranks", "1"])
    two, err2 = run("r2", ["-ranks", "2", "-reduce", "host"])
    assert "4 chunk(s) ran side by side" in err1
    assert err2.count("2 chunk(s) ran side by side") == 2
    assert one == two and "Recomb" in one
    for name in ("r1", "r2"):
        for c in range(4):
            path = tmp_path / ("%s.chunk%d.recomb.gz" % (name, c))
            assert path.exists(), "no local recombination map for chunk %d" % c
            assert len(gzip.open(path, "rt").read().splitlines()) > 1
