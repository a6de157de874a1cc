"""The auxiliary particle filter's look-ahead inside the extend role of the row pipeline of structured models (pf_lookahead.flags
bit 1, load_lookahead(..., structured=True); k_sweep_xmp<..., LOOK>): the path table of the opt-in, and the bits -- against the same
handle on the general kernels (k_extend_mpr -> k_lookahead -> k_decide -> k_resample), against the oracle, across the boundary between
the two paths, in calls of a few rows, in lockstep, and through bin/smcsmc.

Inputs in the style of tests/test_gpu_lookahead_rows.py: make_model(n, E=8, L=1.2e5) made structured with make_structured(P, split_epoch=5,
mig=1.5), make_segments(seed = 20 + n + level, max_seg_len=5000), 400 particles (a partly filled last workgroup of 64), seed 9, the
quantile table of 20 000 prior trees of the structured model.  Every run asserts that it resampled, that a final particle carries a
migration event on a leaf branch (the structured branch of the leaf height in look_factor), that its rows carry doubletons (from three
haplotypes on: two have none) and, from level 3 on, splits."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError, outfile, pf, segments as segmod

pytestmark = pytest.mark.gpu

NP, SEED = 400, 9
COUNT_RTOL = 1e-9
NO_FUSE, K_PIPE = 2, 16      # PF_DEBUG_NO_FUSE, PF_DEBUG_K_PIPE
CASES = [(4, 2, 2, False), (8, 2, 3, False), (6, 3, 4, True), (2, 4, 1, False), (3, 2, 2, False)]
LOCAL = (4, 2, 2, False)     # the case that carries the local recombination map
COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight", "mig_count", "mig_opp", "mig_weight")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _structured(base, P):
    return cases.make_structured(base, P=P, split_epoch=5, mig=1.5)


@functools.lru_cache(maxsize=None)
def _table(n, P):
    return pf.terminal_branch_quantiles(_structured(cases.make_model(n=n, E=8, L=1.2e5), P), seed=1, n_trees=20000)


def _lookahead_of(nsam, segs):
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return segmod.pack_lookahead(rows, nsam)


@functools.lru_cache(maxsize=None)
def _inputs(n, P, level, unphased, seed=None, L=1.2e5):
    base = cases.make_model(n=n, E=8, L=L)
    model = _structured(base, P)
    segs = cases.make_segments(base, seed=20 + n + level if seed is None else seed, unphased=unphased, max_seg_len=5000)
    la = _lookahead_of(n, segs)
    assert n < 3 or (la["n_doubletons"] > 0).any()
    if level >= 3:
        assert (la["first_split_distance"] > 0).any()
    return model, segs, la


def _new(n, P, level, unphased, structured, pipeline=False, model=None, seed=SEED, inputs=None, **kw):
    m, segs, la = inputs if inputs is not None else _inputs(n, P, level, unphased)
    f = ParticleFilter(m if model is None else model, NP, seed=seed, **kw)
    f.init_prior(segs["start"][0]); f.load_segments(segs)
    f.load_lookahead(la, level, _table(n, P), pipeline=pipeline, structured=structured)
    return f


def _snapshot(f, local_recomb=False):
    """everything the comparisons read, taken after finish() (the handle can go)"""
    t = f.trace()
    assert t["resampled"].sum() > 0, "the case must exercise resampling"
    seg, par = f.resample_events()
    out = dict(trace=t, ev_seg=seg, ev_par=par, particles=f.particles(), logl=f.logl(), counts=f.counts(), done=f.segments_done(),
               mig=f.migrations())
    mg = out["mig"]
    on_leaf = [(mg["branch"][i, :mg["n_events"][i]] < f.nsam).any() for i in range(len(mg["n_events"]))]
    assert any(on_leaf), "no final particle with a migration on a leaf branch"
    if local_recomb:
        out["lmap"] = f.local_recomb()
    return out


def _counts_close(ca, cb):
    for k in COUNT_KEYS:
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
    f = _new(n, P, level, unphased, False, local_recomb=local_recomb)
    try:
        assert f.run_path() == "General"
        f.run(); f.finish()
        return _snapshot(f, local_recomb)
    finally:
        f.close()


# ---------------------------------------------------------------- 1. the path
@pytest.mark.parametrize("P,n", [(2, 2), (2, 4), (2, 8), (4, 2)])
def test_the_bit_puts_a_qualifying_structured_handle_on_its_row_pipeline(hiplib, P, n):
    f = _new(n, P, 2, False, True)
    try:
        assert f.run_path() == "SweepXmp" and f.run_path(many=True) == "SweepXmp"
        assert ParticleFilter.can_run_many([f])
        _, _, la = _inputs(n, P, 2, False)
        f.load_lookahead(la, 2, _table(n, P))                         # again, without the bit
        assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many([f])
        f.load_lookahead(la, 2, _table(n, P), structured=True)
        assert f.run_path() == "SweepXmp"
        f.load_lookahead(la, 2, _table(n, P), pipeline=True)          # bit 0 alone means nothing on a structured handle
        assert f.run_path() == "General" and f.run_path(many=True) is None
        f.load_lookahead(la, 2, _table(n, P), pipeline=True, structured=True)
        assert f.run_path() == "SweepXmp"
        f.load_lookahead(la, 0, _table(n, P), structured=True)        # level 0: no look-ahead, whatever the bit
        assert f.run_path() == "SweepXmp" and f.run_path(many=True) == "SweepXmp"
    finally:
        f.close()


def _other_handles():
    focused = lambda m: dict(m, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(8, 2500.0), delay_type=0)   # noqa: E731
    one_pop = lambda m: cases.make_model(n=4, E=8, L=1.2e5)                                                                            # noqa: E731
    return [("one-population", 4, 2, one_pop, {}), ("n9", 9, 2, None, {}), ("focused", 4, 2, focused, {}),
            ("record-trees", 4, 2, None, dict(record_trees=True, gen_cap=64, log_cap=64)),
            ("no-fuse", 4, 2, None, dict(debug=NO_FUSE)), ("k-pipe", 4, 2, None, dict(debug=K_PIPE))]


@pytest.mark.parametrize("n,P,change,kw", [pytest.param(*r[1:], id=r[0]) for r in _other_handles()])
def test_the_bit_leaves_every_other_handle_on_the_general_kernels(hiplib, n, P, change, kw):
    m, _, _ = _inputs(n, P, 2, False)
    f = _new(n, P, 2, False, True, model=None if change is None else change(m), **kw)
    try:
        assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many([f])
    finally:
        f.close()


# ---------------------------------------------------------------- 2. what runs
def test_the_row_pipeline_is_what_runs(hiplib):
    """the launch counters of forty rows, as tests/test_gpu_run_path.py reads them: rows in the extend class, no k_decide, no k_resample
    (on the general kernels the same rows are forty of each)"""
    rows = 40
    got = {}
    for structured in (True, False):
        f = _new(8, 2, 2, False, structured, ess_fraction=0.9)
        try:
            f.set_timing(1)
            f.run(0, rows)
            got[structured] = dict({k: v[1] for k, v in f.kernel_times().items()}, done=f.segments_done(),
                                   resampled=int(np.asarray(f.trace()["resampled"])[:rows].sum()))
        finally:
            f.close()
    assert got[True]["resampled"] >= 3 and got[True]["resampled"] == got[False]["resampled"]
    assert (got[True]["extend"], got[True]["decide"], got[True]["resample"], got[True]["done"]) == (rows, 0, 0, rows)
    assert (got[False]["extend"], got[False]["decide"], got[False]["resample"], got[False]["done"]) == (rows, rows, rows, rows)


# ---------------------------------------------------------------- 3. the bits
@pytest.mark.parametrize("n,P,level,unphased", CASES)
def test_rows_equal_the_general_kernels_and_the_oracle(oracle, hiplib, n, P, level, unphased):
    local = (n, P, level, unphased) == LOCAL
    f = _new(n, P, level, unphased, True, local_recomb=local)
    try:
        assert f.run_path() == "SweepXmp"
        f.run(); f.finish()
        a = _snapshot(f, local)
    finally:
        f.close()
    assert not (_bits(a["particles"]["w_post"]) == _bits(a["particles"]["w_pilot"])).all()      # the factor sits in the pilot weight only
    _same(a, _general(n, P, level, unphased, local))
    model, segs, la = _inputs(n, P, level, unphased)
    o = oracle.Oracle(model, NP, seed=SEED, max_trace_events=64)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.load_lookahead(la, level, _table(n, P))
    o.run(si)
    b = dict(trace=o.trace(), particles=o.particles(), logl=o.logl(), counts=o.counts(), done=len(o.trace()["T"]), mig=o.migrations())
    b["ev_seg"], b["ev_par"] = o.resample_events()
    _same(a, b)


# ---------------------------------------------------------------- 4. across the boundary between the paths
def _boundary(n, P, level, unphased):
    """a row in the middle that follows a resampling row, read off the run on the general kernels"""
    res = np.asarray(_general(n, P, level, unphased)["trace"]["resampled"])
    S = len(res)
    after = [s + 1 for s in range(S // 3, 2 * S // 3) if res[s]]
    assert after, "no resampling row in the middle third"
    return after[len(after) // 2], S


@pytest.mark.parametrize("pipeline_first", [True, False], ids=["rows-then-steps", "steps-then-rows"])
def test_the_factor_crosses_the_boundary_between_the_paths(hiplib, pipeline_first):
    n, P, level, unphased = 8, 2, 3, False
    k, S = _boundary(n, P, level, unphased)
    f = _new(n, P, level, unphased, True)
    try:
        assert f.run_path() == "SweepXmp"
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
    _same(a, _general(n, P, level, unphased))


# ---------------------------------------------------------------- 5. calls of a few rows
def test_calls_of_seven_rows_equal_one_call(hiplib):
    """every call ends with a completion-only launch, which must neither apply a factor nor lose the one it carries"""
    n, P, level, unphased = 6, 3, 4, True
    f = _new(n, P, level, unphased, True)
    try:
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
def _chunk_inputs(k, n=8, P=2, level=2):
    return _inputs(n, P, level, False, seed=50 + k, L=1.2e5 * (0.6 + 0.2 * k))


def test_chunks_in_lockstep_equal_their_own_runs(hiplib):
    n, P, level = 8, 2, 2
    alone = []
    for k in range(3):
        f = _new(n, P, level, False, True, seed=SEED + k, inputs=_chunk_inputs(k))
        try:
            f.run(); f.finish()
            alone.append(_snapshot(f))
        finally:
            f.close()
    many = [_new(n, P, level, False, True, seed=SEED + k, inputs=_chunk_inputs(k)) for k in range(3)]
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
            _counts_same_bits(a["counts"], b["counts"])
    finally:
        for f in many:
            f.close()


def test_groups_that_disagree_in_the_look_ahead_are_refused(hiplib):
    model, segs, _ = _inputs(8, 2, 2, False)
    flagged = _new(8, 2, 2, False, True)
    plain = ParticleFilter(model, NP, seed=SEED)
    plain.init_prior(0.0); plain.load_segments(segs)
    other_level = _new(8, 2, 3, False, True, inputs=_inputs(8, 2, 2, False))
    unflagged = _new(8, 2, 2, False, False)
    # a flagged one-population handle of the same shape (both bits: bit 0 is the one that counts there)
    base = cases.make_model(n=8, E=8, L=1.2e5)
    one_pop = ParticleFilter(base, NP, seed=SEED)
    one_pop.init_prior(0.0); one_pop.load_segments(segs)
    one_pop.load_lookahead(_inputs(8, 2, 2, False)[2], 2, _table(8, 2), pipeline=True, structured=True)
    group = (flagged, plain, other_level, unflagged, one_pop)
    try:
        assert ParticleFilter.can_run_many([flagged]) and ParticleFilter.can_run_many([plain]) and ParticleFilter.can_run_many([other_level])
        assert one_pop.run_path(many=True) == "Sweep" and ParticleFilter.can_run_many([one_pop])
        assert not ParticleFilter.can_run_many([unflagged])
        for refused in ([flagged, plain], [plain, flagged], [flagged, other_level], [flagged, unflagged], [flagged, one_pop], [one_pop, flagged]):
            assert not ParticleFilter.can_run_many(refused)
            with pytest.raises(PfError):
                ParticleFilter.run_many(refused, 0, 5)
    finally:
        for f in group:
            f.close()


# ---------------------------------------------------------------- 7. bin/smcsmc -apf_pipeline
def test_binary_flag_on_a_structured_model(hiplib, built_binary, tmp_path):
    """two populations of four haplotypes each (the two-population command line of tests/golden/cmdlines.json on the first megabase of the
    reference's two-population data), -apf 2 with and without -apf_pipeline: the same counts and opportunities, the same log-likelihood"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seg = os.path.join(root, "tests", "golden", "seg", "twopopssplit_unidirmigr_first2Mb.seg")
    line = [c for c in json.load(open(os.path.join(root, "tests", "golden", "cmdlines.json")))
            if c["num_populations"] == 2 and not c["vb"]][0]
    common = ["-nsam", str(line["num_samples"]), "-Np", "300", "-EM", "0", "-apf", "2", "-tmax", "4", "-lag", "50000", "-seed", "5", "-seg", seg]

    def run(name, extra):
        r = subprocess.run([built_binary] + line["cmdline"].split() + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-400:])
        return outfile.parse_outfile(str(tmp_path / (name + ".out")))

    plain = run("plain", [])
    rows = run("rows", ["-apf_pipeline"])
    assert set(plain) == set(rows)
    assert any(k[0][0] == "Migr" and plain[k] > 0 for k in plain if k[1] == "Count")
    logl = (("LogL", -1, -1, -1, -1), "Count")
    assert plain[logl] == rows[logl] and plain[logl] != 0
    for k in plain:
        if k[1] in ("Opp", "Count"):
            assert rows[k] == pytest.approx(plain[k], rel=1e-9, abs=1e-300), k
