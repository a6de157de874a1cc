"""The auxiliary particle filter's look-ahead inside the extend role of the LDS-tree row pipelines, 9 to 16 haplotypes (pf_lookahead.flags
bit 2, load_lookahead(..., lds=True); k_sweep_xl<false, true> for one population in lockstep, k_sweep_xlmp<false, true> for structured
models made with mp_rows=True): the path table of the opt-in, and the bits -- against the same handle on the general kernels (k_extend /
k_extend_mp -> k_lookahead -> k_decide -> k_resample), against the oracle, across the boundary between the two paths, in calls of a few
rows, in lockstep, and through bin/smcsmc -apf_lds.

Inputs in the style of tests/test_gpu_lookahead_rows_structured.py: make_model(n, E=8, L=1.2e5), made structured with
make_structured(P, split_epoch=5, mig=1.5) for P > 1, make_segments(seed, max_seg_len=5000), particle seed 9, the quantile table of 20 000
prior trees of the model.  400 particles for one population (256 lanes a workgroup: the second workgroup is partly filled and the parent
search crosses workgroups), 300 for structured models (64 lanes: five workgroups, the last partly filled).  Every run asserts that it
resampled, that its rows carry doubletons and, from level 3 on, splits, that w_post and w_pilot differ, and for structured models that a
final particle carries a migration event on a leaf branch.

The segment seeds, chosen by running the oracle on the CPU until a case met all of these (the first candidate, 20 + n + level, did for
every case): (9,1,2) 31, (12,1,3,unphased) 35, (16,1,4) 40, (9,2,2,unphased) 31, (12,3,4) 36, (16,4,3) 39, (16,2,2) 38, (12,2,3) 35,
(12,1,3) 35, (9,3,4,unphased) 33, (12,1,2) 34, (12,2,2) 34; the lockstep chunks 50 + k with particle seed 9 + k.

The case (16, 2, 2) is there for a small mig_cap: the decision's tables then lie behind the state instead of inside the lanes' event
column, and the look-ahead's scratch (columns t0 / t1) must not collide with them.  mig_cap = 16, not 8: with these inputs the oracle
itself stops with "too many migration events on one local tree" at 8, 10, 12 and 14 for every segment seed from 38 to 47, and runs at 16
(seeds 38 and 39).  The tables are still behind the state: they need pipe_lds_doubles(5) > 16 * 64 doubles (their staging area alone is
16 * 64), the event column has mig_cap * 64."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError, pf, segments as segmod, simulate
from test_gpu_run_path import ESS, FORCE_LDS, K_PIPE, NO_FUSE, ROWS, TWO_LAUNCH
from test_gpu_sweep_structured import FRACTIONS

pytestmark = pytest.mark.gpu

SEED = 9
COUNT_RTOL = 1e-9
# (n, P, level, unphased)
CASES = [(9, 1, 2, False), (12, 1, 3, True), (16, 1, 4, False), (9, 2, 2, True), (12, 3, 4, False), (16, 4, 3, False), (16, 2, 2, False)]
LOCAL = (9, 2, 2, True)          # the case that carries the local recombination map
SMALL_CAP = {(16, 2, 2, False): dict(mig_cap=16)}
COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight")
MIG_KEYS = ("mig_count", "mig_opp", "mig_weight")


def _np(P):
    return 400 if P == 1 else 300


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(base, P):
    return base if P == 1 else cases.make_structured(base, P=P, split_epoch=5, mig=1.5)


@functools.lru_cache(maxsize=None)
def _table(n, P):
    return pf.terminal_branch_quantiles(_model(cases.make_model(n=n, E=8, L=1.2e5), P), seed=1, n_trees=20000)


def _lookahead_of(nsam, segs):
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return segmod.pack_lookahead(rows, nsam)


@functools.lru_cache(maxsize=None)
def _inputs(n, P, level, unphased, seed=None, L=1.2e5):
    base = cases.make_model(n=n, E=8, L=L)
    segs = cases.make_segments(base, seed=20 + n + level if seed is None else seed, unphased=unphased, max_seg_len=5000)
    la = _lookahead_of(n, segs)
    assert (la["n_doubletons"] > 0).any()
    if level >= 3:
        assert (la["first_split_distance"] > 0).any()
    return _model(base, P), segs, la


def _new(n, P, level, unphased, lds, model=None, seed=SEED, inputs=None, mp_rows=True, **kw):
    m, segs, la = inputs if inputs is not None else _inputs(n, P, level, unphased)
    if P > 1:
        kw = dict(kw, mp_rows=mp_rows)
    f = ParticleFilter(m if model is None else model, _np(P), seed=seed, **kw)
    f.init_prior(segs["start"][0]); f.load_segments(segs)
    f.load_lookahead(la, level, _table(n, P), lds=lds)
    return f


def _rows(f, s0=0, s1=None):
    """the call that takes a flagged handle's rows on the pipeline: pf_run for structured models, pf_run_many for one population"""
    if f.P > 1:
        f.run(s0, s1)
    else:
        ParticleFilter.run_many([f], s0, f.n_segs if s1 is None else s1)


def _snapshot(f, local_recomb=False):
    """everything the comparisons read, taken after finish() (the handle can go)"""
    t = f.trace()
    assert t["resampled"].sum() > 0, "the case must exercise resampling"
    seg, par = f.resample_events()
    out = dict(trace=t, ev_seg=seg, ev_par=par, particles=f.particles(), logl=f.logl(), counts=f.counts(), done=f.segments_done())
    assert not (_bits(out["particles"]["w_post"]) == _bits(out["particles"]["w_pilot"])).all()      # the factor sits in the pilot weight only
    if f.P > 1:
        mg = out["mig"] = f.migrations()
        on_leaf = [(mg["branch"][i, :mg["n_events"][i]] < f.nsam).any() for i in range(len(mg["n_events"]))]
        assert any(on_leaf), "no final particle with a migration on a leaf branch"
    if local_recomb:
        out["lmap"] = f.local_recomb()
    return out


def _counts_close(ca, cb):
    for k in COUNT_KEYS + (MIG_KEYS if "mig_count" in cb else ()):
        np.testing.assert_allclose(ca[k], cb[k], rtol=COUNT_RTOL, atol=1e-300, err_msg=k)
    assert ca["resample_count"] == cb["resample_count"]


def _counts_same_bits(ca, cb):
    for k in cb:
        assert (_bits(ca[k]) == _bits(cb[k])).all(), k


def _canon_events(mg):
    out = []
    for i in range(len(mg["n_events"])):
        k = mg["n_events"][i]
        out.append(sorted(zip(_bits(mg["times"][i, :k]).tolist(), mg["branch"][i, :k].tolist(), mg["newpop"][i, :k].tolist())))
    return out


def _same(a, b):
    """two snapshots: trace, resampling events and parents, particles, migration lists, node populations and log-likelihood bit for bit;
    the counts (migration statistics included) to 1e-9 -- the pipeline groups those sums by workgroup; the local map by the rule of
    tests/test_gpu_sweep_structured.py::_same"""
    assert a["done"] == b["done"]
    assert (a["trace"]["resampled"] == b["trace"]["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(a["trace"][k]) == _bits(b["trace"][k])).all(), k
    assert (a["ev_seg"] == b["ev_seg"]).all() and (a["ev_par"] == b["ev_par"]).all()
    assert (a["particles"]["children"] == b["particles"]["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(a["particles"][k]) == _bits(b["particles"][k])).all(), k
    assert ("mig" in a) == ("mig" in b)
    if "mig" in a:
        assert (a["mig"]["n_events"] == b["mig"]["n_events"]).all()
        assert (a["mig"]["node_pops"] == b["mig"]["node_pops"]).all()
        assert _canon_events(a["mig"]) == _canon_events(b["mig"])
    assert _bits([a["logl"]])[0] == _bits([b["logl"]])[0]
    _counts_close(a["counts"], b["counts"])
    if "lmap" in a and "lmap" in b:
        for k in a["lmap"]:
            ref = np.asarray(b["lmap"][k], dtype=np.float64)
            np.testing.assert_allclose(a["lmap"][k], ref, rtol=1e-9, atol=1e-12 * max(1e-300, float(np.abs(ref).max())), err_msg=k)


@functools.lru_cache(maxsize=None)
def _general(n, P, level, unphased, local_recomb=False):
    """the same handle without the bit: every row on the general kernels (computed once per case and left unchanged)"""
    kw = SMALL_CAP.get((n, P, level, unphased), {})
    f = _new(n, P, level, unphased, False, local_recomb=local_recomb, **kw)
    try:
        assert f.run_path() == "General" and f.run_path(many=True) is None
        f.run(); f.finish()
        return _snapshot(f, local_recomb)
    finally:
        f.close()


def _paths(f):
    return f.run_path(), f.run_path(many=True), ParticleFilter.can_run_many([f])


# ---------------------------------------------------------------- 1. the path
@pytest.mark.parametrize("n,P", [(9, 1), (12, 1), (16, 1), (12, 2), (9, 3), (16, 4)])
def test_the_bit_puts_a_qualifying_handle_on_its_row_pipeline(hiplib, n, P):
    want = ("General", "SweepXl", True) if P == 1 else ("SweepXlmp", "SweepXlmp", True)
    f = _new(n, P, 2, False, True)
    try:
        assert _paths(f) == want
        _, _, la = _inputs(n, P, 2, False)
        f.load_lookahead(la, 2, _table(n, P))                                    # again, without the bit
        assert _paths(f) == ("General", None, False)
        f.load_lookahead(la, 2, _table(n, P), lds=True)
        assert _paths(f) == want
        f.load_lookahead(la, 2, _table(n, P), pipeline=True, structured=True)     # bits 0 and 1 mean nothing on these handles
        assert _paths(f) == ("General", None, False)
        f.load_lookahead(la, 2, _table(n, P), pipeline=True, structured=True, lds=True)
        assert _paths(f) == want
        f.load_lookahead(la, 0, _table(n, P), lds=True)                           # level 0: the plain rows, whatever the bit
        assert _paths(f) == want
        f.load_lookahead(la, 0, _table(n, P))
        assert _paths(f) == want
    finally:
        f.close()


def _other_handles():
    focused = lambda m: dict(m, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(8, 2500.0), delay_type=0)   # noqa: E731
    trees = dict(record_trees=True, gen_cap=512, log_cap=4096)
    out = [("n8-P1", 8, 1, None, {}), ("n8-P2", 8, 2, None, {}), ("P2-without-mp-rows", 12, 2, None, dict(mp_rows=False)),
           ("focused-P1", 12, 1, focused, {}), ("focused-P2", 12, 2, focused, {}),
           ("record-trees-P1", 12, 1, None, trees), ("record-trees-P2", 12, 2, None, trees)]
    for name, bit in (("force-lds", FORCE_LDS), ("no-fuse", NO_FUSE), ("k-pipe", K_PIPE), ("two-launch", TWO_LAUNCH)):
        out += [(name + "-P1", 12, 1, None, dict(debug=bit)), (name + "-P2", 12, 2, None, dict(debug=bit))]
    return out


@pytest.mark.parametrize("n,P,change,kw", [pytest.param(*r[1:], id=r[0]) for r in _other_handles()])
def test_the_bit_changes_nothing_on_any_other_handle(hiplib, n, P, change, kw):
    m, _, la = _inputs(n, P, 2, False)
    f = _new(n, P, 2, False, False, model=None if change is None else change(m), **kw)
    try:
        without = _paths(f)
        f.load_lookahead(la, 2, _table(n, P), lds=True)
        assert _paths(f) == without
        if n > 8:
            assert without == ("General", None, False)
    finally:
        f.close()


# ---------------------------------------------------------------- 2. what runs
@pytest.mark.parametrize("P", [2, 1])
def test_the_row_pipeline_is_what_runs(hiplib, P):
    """the launch counters of forty rows, as tests/test_gpu_run_path.py::tiny_run reads them: rows in the extend class, no k_decide, no
    k_resample (on the general kernels the same rows are forty of each)"""
    got = {}
    for lds in (True, False):
        f = _new(9, P, 2, False, lds, ess_fraction=ESS)
        try:
            f.set_timing(1)
            if lds:
                _rows(f, 0, ROWS)
            else:
                f.run(0, ROWS)
            got[lds] = dict({k: v[1] for k, v in f.kernel_times().items()}, done=f.segments_done(),
                            resampled=int(np.asarray(f.trace()["resampled"])[:ROWS].sum()))
        finally:
            f.close()
    assert got[True]["resampled"] >= 3 and got[True]["resampled"] == got[False]["resampled"]
    assert (got[True]["extend"], got[True]["decide"], got[True]["resample"], got[True]["done"]) == (ROWS, 0, 0, ROWS)
    assert (got[False]["extend"], got[False]["decide"], got[False]["resample"], got[False]["done"]) == (ROWS, ROWS, ROWS, ROWS)


# ---------------------------------------------------------------- 3. the bits
@pytest.mark.parametrize("n,P,level,unphased", CASES)
def test_rows_equal_the_general_kernels_and_the_oracle(oracle, hiplib, n, P, level, unphased):
    local = (n, P, level, unphased) == LOCAL
    kw = SMALL_CAP.get((n, P, level, unphased), {})
    f = _new(n, P, level, unphased, True, local_recomb=local, **kw)
    try:
        assert f.run_path(many=True) == ("SweepXl" if P == 1 else "SweepXlmp")
        _rows(f); f.finish()
        a = _snapshot(f, local)
    finally:
        f.close()
    _same(a, _general(n, P, level, unphased, local))
    model, segs, la = _inputs(n, P, level, unphased)
    o = oracle.Oracle(model, _np(P), seed=SEED, max_trace_events=64, **kw)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.load_lookahead(la, level, _table(n, P))
    o.run(si)
    b = dict(trace=o.trace(), particles=o.particles(), logl=o.logl(), counts=o.counts(), done=len(o.trace()["T"]))
    if P > 1:
        b["mig"] = o.migrations()
    b["ev_seg"], b["ev_par"] = o.resample_events()
    _same(a, b)


def test_the_small_mig_cap_case_is_what_its_docstring_says(oracle):
    """(16, 2, 2) with mig_cap = 16: the library plans the handle with that capacity and the rings of k_sweep_xlmp, the decision's tables
    (pipe_lds_doubles of pf_pipe.h, restated here: five wavefronts of particles, PF_PIPE_BS = 256, PF_PIPE_STAGE = 16) are longer than the
    lanes' event column, so mp_pipe_tables_inside is false and they lie behind the state; and mig_cap = 8, the issue's figure, stops the
    oracle itself on these inputs"""
    case = (16, 2, 2, False)
    model, segs, la = _inputs(*case)
    p = pf.plan(model, _np(2), seed=SEED, mp_rows=True, **SMALL_CAP[case])
    assert p["rings"] == "Xlmp" and p["mcap"] == SMALL_CAP[case]["mig_cap"] == 16
    nc = (_np(2) + 63) // 64
    ncpad = (nc + 63) // 64 * 64
    tables = ncpad + (ncpad + 1) + 3 * 64 + 256 // 64 + 16 * 64 + (256 + 3 * (256 // 64) + 1) // 2 + 2
    assert nc == 5 and tables == 1485 and tables > p["mcap"] * 64                  # mp_pipe_tables_inside(mcap, nc) is false
    assert tables <= pf.plan(model, _np(2), seed=SEED, mp_rows=True)["mcap"] * 64    # (with the default capacity they are inside)
    with pytest.raises(RuntimeError, match="too many migration events on one local tree"):
        o = oracle.Oracle(model, _np(2), seed=SEED, max_trace_events=64, mig_cap=8)
        o.init_prior(segs["start"][0])
        si = o.pack_segments(model, segs)
        o.load_lookahead(la, 2, oracle.terminal_branch_quantiles(model, seed=1, n_trees=2000))
        o.run(si)


# ---------------------------------------------------------------- 4. across the boundary between the paths
def _boundary(n, P, level, unphased):
    """a row in the middle that follows a resampling row, read off the run on the general kernels"""
    res = np.asarray(_general(n, P, level, unphased)["trace"]["resampled"])
    S = len(res)
    after = [s + 1 for s in range(S // 3, 2 * S // 3) if res[s]]
    assert after, "no resampling row in the middle third"
    return after[len(after) // 2], S


@pytest.mark.parametrize("pipeline_first", [True, False], ids=["rows-then-steps", "steps-then-rows"])
@pytest.mark.parametrize("P", [2, 1])
def test_the_factor_crosses_the_boundary_between_the_paths(hiplib, P, pipeline_first):
    n, level, unphased = 12, 3, False
    k, S = _boundary(n, P, level, unphased)
    f = _new(n, P, level, unphased, True)
    try:
        assert f.run_path(many=True) == ("SweepXl" if P == 1 else "SweepXlmp")
        def steps(s0, s1):
            for s in range(s0, s1):
                f.update_segment(s); f.count(s); f.resample(s)
        if pipeline_first:
            _rows(f, 0, k); steps(k, S)
        else:
            steps(0, k); _rows(f, k, S)
        f.finish()
        a = _snapshot(f)
    finally:
        f.close()
    _same(a, _general(n, P, level, unphased))


# ---------------------------------------------------------------- 5. calls of a few rows
def test_calls_of_seven_rows_equal_one_call(hiplib):
    """every call ends with a completion-only launch, which must neither apply a factor nor lose the one it carries"""
    n, P, level, unphased = 9, 3, 4, True
    f = _new(n, P, level, unphased, True)
    try:
        assert f.run_path() == "SweepXlmp"
        S = f.n_segs
        for s0 in range(0, S, 7):
            f.run(s0, min(S, s0 + 7))
        f.finish()
        a = _snapshot(f)
    finally:
        f.close()
    g = _new(n, P, level, unphased, True)
    try:
        g.run(); g.finish()
        b = _snapshot(g)
    finally:
        g.close()
    _same(a, b)
    _counts_same_bits(a["counts"], b["counts"])                   # the same path in both: the counts too are the same bits
    _same(a, _general(n, P, level, unphased))


# ---------------------------------------------------------------- 6. lockstep
def _chunk_inputs(k, n, P, level=2):
    return _inputs(n, P, level, False, seed=50 + k, L=1.2e5 * FRACTIONS[k])


@pytest.mark.parametrize("P", [1, 2])
def test_chunks_in_lockstep_equal_their_own_runs_on_the_general_kernels(hiplib, P):
    n, level = 12, 2
    alone = []
    for k in range(len(FRACTIONS)):
        f = _new(n, P, level, False, False, seed=SEED + k, inputs=_chunk_inputs(k, n, P))
        try:
            assert f.run_path() == "General"
            f.run(); f.finish()
            alone.append(_snapshot(f))
        finally:
            f.close()
    many = [_new(n, P, level, False, True, seed=SEED + k, inputs=_chunk_inputs(k, n, P)) for k in range(len(FRACTIONS))]
    try:
        assert ParticleFilter.can_run_many(many)
        assert many[0].run_path(many=True) == ("SweepXl" if P == 1 else "SweepXlmp")
        assert len({f.n_segs for f in many}) == len(many)           # the chunks do not end together
        nmax = max(f.n_segs for f in many)
        for s0 in range(0, nmax, 29):                               # chunks that are done sit the later calls out
            ParticleFilter.run_many(many, s0, min(nmax, s0 + 29))
        for f in many:
            f.finish()
        for f, b in zip(many, alone):
            _same(_snapshot(f), b)
    finally:
        for f in many:
            f.close()


@pytest.mark.parametrize("P", [1, 2])
def test_groups_that_disagree_are_refused(hiplib, P):
    n = 12
    flagged = _new(n, P, 2, False, True)
    unflagged = _new(n, P, 2, False, False)
    both_bits = ParticleFilter(_inputs(n, P, 2, False)[0], _np(P), seed=SEED, **(dict(mp_rows=True) if P > 1 else {}))
    both_bits.init_prior(0.0); both_bits.load_segments(_inputs(n, P, 2, False)[1])
    both_bits.load_lookahead(_inputs(n, P, 2, False)[2], 2, _table(n, P), pipeline=True, lds=True)      # other flags: another group
    other_level = _new(n, P, 3, False, True, inputs=_inputs(n, P, 2, False))
    plain = ParticleFilter(_inputs(n, P, 2, False)[0], _np(P), seed=SEED, **(dict(mp_rows=True) if P > 1 else {}))
    plain.init_prior(0.0); plain.load_segments(_inputs(n, P, 2, False)[1])
    group = [flagged, unflagged, both_bits, other_level, plain]
    refused = [[flagged, unflagged], [unflagged, flagged], [flagged, both_bits], [flagged, other_level], [flagged, plain], [plain, flagged]]
    if P > 1:
        no_rows = _new(n, P, 2, False, True, mp_rows=False)
        group.append(no_rows)
        refused += [[flagged, no_rows], [no_rows, flagged]]
    try:
        for f in (flagged, both_bits, other_level, plain):
            assert ParticleFilter.can_run_many([f])
        assert not ParticleFilter.can_run_many([unflagged])
        for r in refused:
            assert not ParticleFilter.can_run_many(r)
            with pytest.raises(PfError):
                ParticleFilter.run_many(r, 0, 5)
    finally:
        for f in group:
            f.close()


# ---------------------------------------------------------------- 7. bin/smcsmc -apf_lds
def _binary_run(binary, tmp_path, core, common, name, extra):
    r = subprocess.run([binary] + core + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stderr[-2000:])
    return open(tmp_path / (name + ".out")).read(), r.stdout + r.stderr


def test_binary_flag_on_a_structured_model(hiplib, built_binary, tmp_path):
    """the .seg and command line of tests/test_gpu_sweep_structured_lds.py::test_binary_mp_rows_chunks_side_by_side (two populations of
    six haplotypes each) with -apf 2: -mp_rows -apf_lds changes no character of the .out, and two chunks then share their launches"""
    n, L, Np = 12, 240000, 160
    base = cases.make_model(n=n, E=8, L=float(L))
    seg = str(tmp_path / "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(L), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=40 + n))
    core = ("-N0 10000 -t %g -r %g %d -I 2 6 6 -eN 0.0 1.0 -ema 0.0 0 2.0 2.0 0 -eN 0.1 1.0 -ema 0.1 0 2.0 2.0 0 "
            "-eN 0.5 1.0 -ema 0.5 0 0 0 0 -ej 0.5 2 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", str(Np), "-seed", "5", "-lag", "50000", "-apf", "2", "-ranks", "1"]
    plain, _ = _binary_run(built_binary, tmp_path, core, common, "plain", [])
    rows, _ = _binary_run(built_binary, tmp_path, core, common, "rows", ["-mp_rows", "-apf_lds"])
    assert rows == plain and "Migr" in plain
    chunks, log0 = _binary_run(built_binary, tmp_path, core, common, "chunks", ["-chunks", "2", "-mp_rows"])
    chunks_rows, log1 = _binary_run(built_binary, tmp_path, core, common, "chunks_rows", ["-chunks", "2", "-mp_rows", "-apf_lds"])
    assert "ran one after the other" in log0 and "2 chunk(s) ran side by side" in log1
    assert chunks_rows == chunks


def test_binary_flag_on_one_population(hiplib, built_binary, tmp_path):
    """ten haplotypes of one population, -chunks 2 -apf 2: one after the other without -apf_lds (with -apf_pipeline too, which means nothing
    at this size), side by side with it, and no character of the .out changes"""
    n, L, Np = 10, 240000, 300
    base = cases.make_model(n=n, E=8, L=float(L))
    seg = str(tmp_path / "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(L), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=40 + n))
    core = ("-N0 10000 -t %g -r %g %d -eN 0 1 -eN 0.01 1 -eN 0.25 1 -eN 1 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", str(Np), "-seed", "4", "-lag", "20000", "-apf", "2", "-ranks", "1", "-chunks", "2"]
    chunks, log0 = _binary_run(built_binary, tmp_path, core, common, "chunks", [])
    old_flag, log1 = _binary_run(built_binary, tmp_path, core, common, "old_flag", ["-apf_pipeline"])
    chunks_rows, log2 = _binary_run(built_binary, tmp_path, core, common, "chunks_rows", ["-apf_lds"])
    assert "ran one after the other" in log0 and "ran side by side" not in log0
    assert "2 chunk(s) ran one after the other" in log1
    assert "2 chunk(s) ran side by side" in log2
    assert chunks_rows == chunks and old_flag == chunks
