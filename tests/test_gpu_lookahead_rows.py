"""The auxiliary particle filter's look-ahead inside the extend role of the row pipeline (pf_lookahead.flags bit 0,
load_lookahead(..., pipeline=True); k_sweep<..., LOOK>): the path table of the opt-in, and the bits -- against the same handle on the
general kernels (k_extend_reg -> k_lookahead -> k_decide -> k_resample), against the oracle, across the boundary between the two
paths, in calls of a few rows, in lockstep, and through bin/smcsmc.

Inputs are those of tests/test_gpu_parity.py::test_auxiliary_particle_filter_parity: make_model(n, E=8, L=1.2e5), make_segments(seed =
20 + n + level, max_seg_len=5000, a missing block at level 2), 400 particles (a partly filled second workgroup), seed 9, the quantile table
of 20 000 prior trees.  Every run asserts that it resampled and that its rows carry doubletons (from three haplotypes on: two have none)
and, from level 3 on, splits."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, pf, segments as segmod

pytestmark = pytest.mark.gpu

NP, SEED = 400, 9
COUNT_RTOL = 1e-9
NO_FUSE = 2          # PF_DEBUG_NO_FUSE
CASES = [(4, 1, False), (4, 2, True), (6, 2, False), (8, 3, False), (8, 4, True), (2, 2, False)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _table(n):
    return pf.terminal_branch_quantiles(cases.make_model(n=n, E=8, L=1.2e5), seed=1, n_trees=20000)


def _lookahead_of(model, segs):
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return segmod.pack_lookahead(rows, model["nsam"])


@functools.lru_cache(maxsize=None)
def _inputs(n, level, unphased, seed=None, L=1.2e5):
    model = cases.make_model(n=n, E=8, L=L)
    segs = cases.make_segments(model, seed=20 + n + level if seed is None else seed, unphased=unphased, max_seg_len=5000,
                               missing_block=(40000, 60000, (0, 1)) if level == 2 else None)
    la = _lookahead_of(model, segs)
    # (two haplotypes have no doubletons, whatever the data: a site where both carry the mutation does not segregate.  The n = 2 cases
    # run all the same -- singletons, the missing block -- and assert this for nothing)
    assert n == 2 or (la["n_doubletons"] > 0).any()
    if level >= 3:
        assert (la["first_split_distance"] > 0).any()
    return model, segs, la


def _new(n, level, unphased, pipeline, model=None, Np=NP, seed=SEED, inputs=None, **kw):
    base, segs, la = inputs if inputs is not None else _inputs(n, level, unphased)
    f = ParticleFilter(base if model is None else model, Np, seed=seed, **kw)
    f.init_prior(segs["start"][0]); f.load_segments(segs)
    f.load_lookahead(la, level, _table(n), pipeline=pipeline)
    return f


def _snapshot(f, local_recomb=False):
    """everything the comparisons read, taken after finish() (the handle can go)"""
    t = f.trace()
    assert t["resampled"].sum() > 0, "the case must exercise resampling"
    seg, par = f.resample_events()
    out = dict(trace=t, ev_seg=seg, ev_par=par, particles=f.particles(), logl=f.logl(), counts=f.counts(), done=f.segments_done())
    if local_recomb:
        out["lmap"] = f.local_recomb()
    return out


def _counts_close(ca, cb):
    for k in ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight"):
        np.testing.assert_allclose(ca[k], cb[k], rtol=COUNT_RTOL, atol=1e-300, err_msg=k)
    assert ca["resample_count"] == cb["resample_count"]
    np.testing.assert_allclose(ca["delayed_opp"], cb["delayed_opp"], rtol=1e-12)


def _same(a, b):
    """two snapshots: trace, resampling events and parents, particles and log-likelihood bit for bit; the counts (and the local map) to
    1e-9 of the column scale -- the pipeline groups those sums by workgroup"""
    assert a["done"] == b["done"]
    assert (a["trace"]["resampled"] == b["trace"]["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(a["trace"][k]) == _bits(b["trace"][k])).all(), k
    assert (a["ev_seg"] == b["ev_seg"]).all() and (a["ev_par"] == b["ev_par"]).all()
    assert (a["particles"]["children"] == b["particles"]["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(a["particles"][k]) == _bits(b["particles"][k])).all(), k
    assert _bits([a["logl"]])[0] == _bits([b["logl"]])[0]
    _counts_close(a["counts"], b["counts"])
    if "lmap" in a and "lmap" in b:
        for k in a["lmap"]:
            np.testing.assert_allclose(a["lmap"][k], b["lmap"][k], rtol=COUNT_RTOL, atol=COUNT_RTOL * max(1e-300, float(np.abs(b["lmap"][k]).max())))


def _general(n, level, unphased, local_recomb=False):
    """the same handle without the bit: every row on the general kernels (computed once per case)"""
    return _general_run(n, level, unphased, bool(local_recomb))


@functools.lru_cache(maxsize=None)
def _general_run(n, level, unphased, local_recomb):
    f = _new(n, level, unphased, False, local_recomb=local_recomb)
    try:
        assert f.run_path() == "General"
        f.run(); f.finish()
        return _snapshot(f, local_recomb)
    finally:
        f.close()


# ---------------------------------------------------------------- 1. the path
@pytest.mark.parametrize("n", [2, 4, 6, 8])
def test_the_bit_puts_a_qualifying_handle_on_the_sweep(hiplib, n):
    f = _new(n, 2, False, True)
    try:
        assert f.run_path() == "Sweep" and f.run_path(many=True) == "Sweep"
        assert ParticleFilter.can_run_many([f])
        _, _, la = _inputs(n, 2, False)
        f.load_lookahead(la, 2, _table(n))                       # again, without the bit
        assert f.run_path() == "General" and f.run_path(many=True) is None
        f.load_lookahead(la, 2, _table(n), pipeline=True)
        assert f.run_path() == "Sweep"
        f.load_lookahead(la, 0, _table(n), pipeline=True)        # level 0: no look-ahead, whatever the bit
        assert f.run_path() == ("SweepSplit" if n <= 4 else "Sweep")
    finally:
        f.close()


def _other_handles():
    focused = lambda m: dict(m, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(8, 2500.0), delay_type=0)   # noqa: E731
    two_pops = lambda m: cases.make_structured(m, P=2, split_epoch=7, mig=2.0)                                                          # noqa: E731
    return [("n9", 9, None, {}), ("P2", 4, two_pops, {}), ("focused", 4, focused, {}),
            ("record-trees", 4, None, dict(record_trees=True, gen_cap=64, log_cap=64)),
            ("no-fuse", 4, None, dict(debug=NO_FUSE)), ("131073-particles", 2, None, dict(Np=131073, gen_cap=32, log_cap=32))]


@pytest.mark.parametrize("n,change,kw", [pytest.param(*r[1:], id=r[0]) for r in _other_handles()])
def test_the_bit_leaves_every_other_handle_on_the_general_kernels(hiplib, n, change, kw):
    base, _, _ = _inputs(n, 2, False)
    f = _new(n, 2, False, True, model=None if change is None else change(base), **kw)
    try:
        assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many([f])
    finally:
        f.close()


def test_the_sweep_is_what_runs(hiplib):
    """the launch counters of forty rows, as tests/test_gpu_run_path.py reads them: rows in the extend class, no k_decide, no k_resample
    (on the general kernels the same rows are forty of each)"""
    rows = 40
    got = {}
    for pipeline in (True, False):
        f = _new(8, 2, False, pipeline, ess_fraction=0.9)
        try:
            f.set_timing(1)
            f.run(0, rows)
            got[pipeline] = dict({k: v[1] for k, v in f.kernel_times().items()}, done=f.segments_done(),
                                 resampled=int(np.asarray(f.trace()["resampled"])[:rows].sum()))
        finally:
            f.close()
    assert got[True]["resampled"] >= 3 and got[True]["resampled"] == got[False]["resampled"]
    assert (got[True]["extend"], got[True]["decide"], got[True]["resample"], got[True]["done"]) == (rows, 0, 0, rows)
    assert (got[False]["extend"], got[False]["decide"], got[False]["resample"], got[False]["done"]) == (rows, rows, rows, rows)


# ---------------------------------------------------------------- 2. the bits
@pytest.mark.parametrize("n,level,unphased", CASES)
def test_rows_equal_the_general_kernels_and_the_oracle(oracle, hiplib, n, level, unphased):
    local = (n, level) == (6, 2)                                  # the local recombination map rides along in one case
    f = _new(n, level, unphased, True, local_recomb=local)
    try:
        assert f.run_path() == "Sweep"
        f.run(); f.finish()
        a = _snapshot(f, local)
    finally:
        f.close()
    _same(a, _general(n, level, unphased, local))
    model, segs, la = _inputs(n, level, unphased)
    o = oracle.Oracle(model, NP, seed=SEED, max_trace_events=64)
    if local:
        o.enable_local_recomb()
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.load_lookahead(la, level, _table(n))
    o.run(si)
    b = dict(trace=o.trace(), particles=o.particles(), logl=o.logl(), counts=o.counts(), done=len(o.trace()["T"]))
    b["ev_seg"], b["ev_par"] = o.resample_events()
    _same(a, b)
    if local:
        # against the oracle by the rule of tests/test_gpu_parity.py::test_local_recombination_map_parity: the cumulated opportunity (the
        # differential form cancels large terms), and the counts to 1e-9 of the column scale
        lo, lg = o.local_recomb(model["loci_length"]), a["lmap"]
        co, cg = np.cumsum(lo["opp_diff"]), np.cumsum(lg["opp_diff"])
        assert co.max() > 0 and lo["counts"][:n].sum() > 0
        np.testing.assert_allclose(cg, co, rtol=1e-7, atol=1e-7 * co.max())
        np.testing.assert_allclose(lg["counts"], lo["counts"], rtol=COUNT_RTOL, atol=1e-12 * max(1.0, lo["counts"].max()))


# ---------------------------------------------------------------- 3. across the boundary between the paths
def _boundary(n, level, unphased):
    """a row in the middle that follows a resampling row, read off the run on the general kernels"""
    res = np.asarray(_general(n, level, unphased)["trace"]["resampled"])
    S = len(res)
    after = [s + 1 for s in range(S // 3, 2 * S // 3) if res[s]]
    assert after, "no resampling row in the middle third"
    return after[len(after) // 2], S


@pytest.mark.parametrize("pipeline_first", [True, False], ids=["rows-then-steps", "steps-then-rows"])
def test_the_factor_crosses_the_boundary_between_the_paths(hiplib, pipeline_first):
    n, level, unphased = 8, 3, False
    k, S = _boundary(n, level, unphased)
    f = _new(n, level, unphased, True)
    try:
        assert f.run_path() == "Sweep"
        def steps(s0, s1):
            for s in range(s0, s1):
                f.update_segment(s); f.count(s); f.resample(s)
        if pipeline_first:
            f.run(0, k); steps(k, S)
        else:
            steps(0, k); f.run(k, None)
        f.finish()
        a = _snapshot(f)
    finally:
        f.close()
    _same(a, _general(n, level, unphased))


# ---------------------------------------------------------------- 4. calls of a few rows
def test_calls_of_seven_rows_equal_one_call(hiplib):
    """every call ends with a completion-only launch, which must neither apply a factor nor lose the one it carries"""
    n, level, unphased = 4, 2, True
    f = _new(n, level, unphased, True)
    try:
        S = f.n_segs
        for s0 in range(0, S, 7):
            f.run(s0, min(S, s0 + 7))
        f.finish()
        a = _snapshot(f)
    finally:
        f.close()
    g = _new(n, level, unphased, True)
    try:
        g.run(); g.finish()
        b = _snapshot(g)
    finally:
        g.close()
    _same(a, b)
    for k in b["counts"]:                                        # the same path in both: the counts too are the same bits
        assert (_bits(a["counts"][k]) == _bits(b["counts"][k])).all(), k
    _same(a, _general(n, level, unphased))


# ---------------------------------------------------------------- 5. lockstep
def _chunk_inputs(k, n=8, level=2):
    return _inputs(n, level, False, seed=50 + k, L=1.2e5 * (0.6 + 0.2 * k))


def test_chunks_in_lockstep_equal_their_own_runs(hiplib):
    n, level = 8, 2
    alone = []
    for k in range(3):
        f = _new(n, level, False, True, seed=SEED + k, inputs=_chunk_inputs(k))
        try:
            f.run(); f.finish()
            alone.append(_snapshot(f))
        finally:
            f.close()
    many = [_new(n, level, False, True, seed=SEED + k, inputs=_chunk_inputs(k)) for k in range(3)]
    try:
        assert ParticleFilter.can_run_many(many)
        assert len({f.n_segs for f in many}) == 3                # the chunks do not end together
        nmax = max(f.n_segs for f in many)
        for i, s0 in enumerate(range(0, nmax, 11)):
            s1 = min(nmax, s0 + 11)
            if i == 2:
                # one handle goes a call alone between two lockstep calls; the others catch up in a group of two
                many[1].run(s0, min(many[1].n_segs, s1))
                ParticleFilter.run_many([many[0], many[2]], s0, s1)
            else:
                ParticleFilter.run_many(many, s0, s1)
        for f in many:
            f.finish()
        for f, b in zip(many, alone):
            a = _snapshot(f)
            _same(a, b)
            for k in b["counts"]:
                assert (_bits(a["counts"][k]) == _bits(b["counts"][k])).all(), k
    finally:
        for f in many:
            f.close()


def test_groups_that_disagree_in_the_look_ahead_are_refused(hiplib):
    flagged = _new(8, 2, False, True)
    plain = ParticleFilter(_inputs(8, 2, False)[0], NP, seed=SEED)
    plain.init_prior(0.0); plain.load_segments(_inputs(8, 2, False)[1])
    other_level = _new(8, 3, False, True, inputs=_inputs(8, 2, False))
    unflagged = _new(8, 2, False, False)
    four = _new(4, 2, False, True)
    try:
        assert ParticleFilter.can_run_many([flagged]) and ParticleFilter.can_run_many([plain]) and ParticleFilter.can_run_many([other_level])
        assert not ParticleFilter.can_run_many([flagged, plain]) and not ParticleFilter.can_run_many([plain, flagged])
        assert not ParticleFilter.can_run_many([flagged, other_level])
        assert not ParticleFilter.can_run_many([flagged, unflagged])
        # four haplotypes beside eight: refused by the rule for plain handles (sweep_compatible: the chunks of a group have the same number of
        # haplotypes), which the look-ahead does not change
        assert ParticleFilter.can_run_many([four]) and not ParticleFilter.can_run_many([flagged, four])
        with pytest.raises(pf.PfError):
            ParticleFilter.run_many([flagged, plain], 0, 5)
    finally:
        for f in (flagged, plain, other_level, unflagged, four):
            f.close()


# ---------------------------------------------------------------- 6. bin/smcsmc -apf_pipeline
def test_binary_flag_changes_no_character(hiplib, tmp_path):
    """the small .seg and command line of tests/test_gpu_parity.py::test_binary_auxiliary_particle_filter"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "bin", "smcsmc")
    seg = os.path.join(root, "tests", "golden", "seg", "constpopsize_first3000.seg")
    L = 1000000
    core = ("-N0 10000 -t %g -r %g %d -eN 0 1 -eN 0.01 1 -eN 0.25 1 -eN 1 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", "2", "-Np", "300", "-EM", "0", "-tmax", "4", "-lag", "20000", "-seed", "4", "-apf", "2", "-seg", seg]

    def run(name, extra):
        r = subprocess.run([binary] + core + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-400:])
        return open(tmp_path / (name + ".out")).read(), r.stdout + r.stderr

    plain, _ = run("plain", [])
    rows, _ = run("rows", ["-apf_pipeline"])
    assert rows == plain
    chunks, log0 = run("chunks", ["-chunks", "2"])
    chunks_rows, log1 = run("chunks_rows", ["-chunks", "2", "-apf_pipeline"])
    assert "ran one after the other" in log0 and "ran side by side" in log1
    assert chunks_rows == chunks
