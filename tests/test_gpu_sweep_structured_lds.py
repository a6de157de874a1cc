"""Structured models of 9 to 16 haplotypes on the row pipeline (pf_params.flags bit 3, ParticleFilter(..., mp_rows=True)): the extend role
k_sweep_xlmp keeps tree and migration list in LDS, the other roles are k_sweep_blc<16, 2 or 4, *>; two launches a row, alone (pf_run)
and in lockstep (pf_run_many).  The path must give the oracle's bits, be the one pf_get_run_path names, give every chunk of a lockstep
group the bits of its own run, refuse the groups it cannot serve, and report a ring that is too small.  Off unless asked for: a handle
without the flag, and every handle the flag has no meaning for, keeps the path it had."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError
from test_gpu_run_path import FORCE_LDS, PF_RING, tiny_run
from test_gpu_structured import _assert_counts_close, _assert_state_equal
from test_gpu_sweep_structured import CALL, FRACTIONS, _bits, _lockstep, _same, _snap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCUS = dict(bias_heights=[400.0], bias_strengths=[4.0, 1.0], delay_type=0)

# (n, E, P, Np, seed, focused): Np = 130 and 300 leave the last 64-particle workgroup partly filled, P = 3 runs on the instances of four
SHAPES = [(9, 8, 2, 300, 3, False), (12, 6, 3, 256, 4, False), (16, 8, 4, 192, 5, False), (16, 8, 2, 130, 6, False),
          (10, 8, 2, 200, 7, True), (16, 6, 4, 128, 8, True)]


def _inputs(n, E, P, seed, focused, L=1.0e5, lag=None):
    base = cases.make_model(n=n, E=E, L=L) if lag is None else cases.make_model(n=n, E=E, L=L, lag=lag)
    segs = cases.make_segments(base, seed=seed, max_seg_len=5000)
    model = cases.make_structured(base, P=P, split_epoch=E - 3, mig=2.0)
    if focused:
        model = dict(model, application_delays=np.full(E, 2500.0), **FOCUS)
    return model, segs


class _Frozen:
    """what the comparisons read of an oracle run, kept so that the oracle runs once per input"""
    def __init__(self, o):
        self._p, self._m, self._t, self._r, self._c, self._l = o.particles(), o.migrations(), o.trace(), o.resample_events(), o.counts(), o.logl()

    def particles(self): return self._p
    def migrations(self): return self._m
    def trace(self): return self._t
    def resample_events(self): return self._r
    def counts(self): return self._c
    def logl(self): return self._l


@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, n, E, P, Np, seed, focused, L=1.0e5, lag=None):
    model, segs = _inputs(n, E, P, seed, focused, L, lag)
    o = oracle.Oracle(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64)
    o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    return _Frozen(o)


def _flagged(model, segs, Np, seed, **kw):
    g = ParticleFilter(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=64, mp_rows=True, **kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    return g


def _assert_oracle_parity(o, g):
    to, tg = o.trace(), g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all()
    assert to["resampled"].sum() > 0, "the case must resample"
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    assert _bits(o.logl()) == _bits(g.logl())
    so, po = o.resample_events(); sg, pg = g.resample_events()
    assert (so == sg).all() and (po == pg).all()
    _assert_state_equal(o, g)
    co, cg = o.counts(), g.counts()
    assert co["mig_count"].sum() > 0
    _assert_counts_close(co, cg)


# ---------------------------------------------------------------- 1. oracle parity, alone
@pytest.mark.parametrize("n,E,P,Np,seed,focused", SHAPES, ids=["n%d-E%d-P%d-Np%d%s" % (s[0], s[1], s[2], s[3], "-focused" if s[5] else "") for s in SHAPES])
def test_the_flagged_path_gives_the_oracles_bits(oracle, hiplib, n, E, P, Np, seed, focused):
    model, segs = _inputs(n, E, P, seed, focused)
    g = _flagged(model, segs, Np, seed)
    try:
        assert g.run_path() == "SweepXlmp"
        g.run(); g.finish()
        _assert_oracle_parity(_oracle_run(oracle, n, E, P, Np, seed, focused), g)
    finally:
        g.close()


# ---------------------------------------------------------------- 2. the path is the one named
def test_the_named_path_is_the_one_that_runs(hiplib):
    kw = dict(n=9, P=2, mp_rows=True)
    for many in (False, True):
        got = tiny_run(kw, many)
        assert got["resampled"] >= 3 and got["done"] == 40
        assert (got["extend"], got["decide"], got["resample"]) == (40, 0, 0), got


def _paths(f):
    return f.run_path(), f.run_path(many=True), ParticleFilter.can_run_many([f])


def test_run_path_with_and_without_the_flag(hiplib):
    model, segs = _inputs(9, 8, 2, 3, False)
    with_flag = _flagged(model, segs, 128, 1)
    without = ParticleFilter(model, 128, seed=1)
    without.init_prior(0.0); without.load_segments(segs)
    try:
        assert _paths(with_flag) == ("SweepXlmp", "SweepXlmp", True)
        assert _paths(without) == ("General", None, False)
    finally:
        with_flag.close(); without.close()


NOT_QUALIFYING = [
    ("P2-n8", dict(n=8, P=2), {}, ("SweepXmp", "SweepXmp", True)),
    ("P1-n12", dict(n=12, P=1), {}, ("General", "SweepXl", True)),
    ("record-trees", dict(n=12, P=2), dict(record_trees=True, gen_cap=512, log_cap=4096), ("General", None, False)),
    ("force-lds", dict(n=12, P=2), dict(debug=FORCE_LDS), ("General", None, False)),
]


@pytest.mark.parametrize("shape,kw,want", [pytest.param(*r[1:], id=r[0]) for r in NOT_QUALIFYING])
def test_the_flag_means_nothing_on_a_handle_that_does_not_qualify(hiplib, shape, kw, want):
    base = cases.make_model(n=shape["n"], E=6, L=4e4)
    segs = cases.make_segments(base, seed=2, max_seg_len=4000)
    model = base if shape["P"] == 1 else cases.make_structured(base, P=shape["P"], split_epoch=4, mig=1.5)
    got = []
    for mp_rows in (True, False):
        f = ParticleFilter(model, 128, seed=1, mp_rows=mp_rows, **kw)
        f.init_prior(0.0); f.load_segments(segs)
        got.append(_paths(f))
        f.close()
    assert got[0] == got[1] == want


def test_a_short_generation_ring_is_refused_with_and_without_the_flag(hiplib):
    """gen_cap = PF_RING + 3: pf_create refuses every structured model with such a ring, and the flag does not change that"""
    model, segs = _inputs(9, 8, 2, 3, False)
    texts = []
    for mp_rows in (True, False):
        with pytest.raises(PfError, match="gen_cap must be at least 20") as e:
            ParticleFilter(model, 128, seed=1, gen_cap=PF_RING + 3, mp_rows=mp_rows)
        texts.append(str(e.value))
    assert texts[0] == texts[1]


def test_a_look_ahead_takes_the_handle_to_the_general_kernels(hiplib):
    from smcsmc_amd import pf, segments as segmod
    n = 12
    base = cases.make_model(n=n, E=6, L=4e4)
    segs = cases.make_segments(base, seed=2, max_seg_len=4000)
    model = cases.make_structured(base, P=2, split_epoch=4, mig=1.5)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, al))) for s, l, st, al in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    la = segmod.pack_lookahead(rows, n)
    tbl = pf.terminal_branch_quantiles(model, seed=1, n_trees=2000)
    f = _flagged(model, segs, 128, 1)
    try:
        assert _paths(f) == ("SweepXlmp", "SweepXlmp", True)
        for kw in (dict(), dict(pipeline=True, structured=True)):
            f.load_lookahead(la, 2, tbl, **kw)
            assert _paths(f) == ("General", None, False)
        f.load_lookahead(la, 0, tbl)
        assert _paths(f) == ("SweepXlmp", "SweepXlmp", True)
    finally:
        f.close()


# ---------------------------------------------------------------- 3. lockstep equals alone
LOCK = [(12, 2, 320, False), (16, 4, 200, False), (9, 2, 256, True)]
HEAD = LOCK[0]


@functools.lru_cache(maxsize=None)
def _chunks(n, P, focused):
    """four chunks of one model: lengths 0.5, 0.7, 0.85 and 1.0 x 1.2e5, each with its own data (tests/test_gpu_sweep_structured.py)"""
    out = []
    for k, frac in enumerate(FRACTIONS):
        base = cases.make_model(n=n, E=8, L=1.2e5 * frac)
        segs = cases.make_segments(base, seed=50 + 10 * n + 3 * k, max_seg_len=4000)
        model = cases.make_structured(base, P=P, split_epoch=5, mig=1.5)
        if focused:
            model = dict(model, application_delays=np.full(8, 2500.0), **FOCUS)
        out.append((model, segs))
    return out


def _new(model, segs, Np, seed, **kw):
    f = ParticleFilter(model, Np, seed=seed, local_recomb=True, mp_rows=True, **kw)
    f.init_prior(0.0); f.load_segments(segs)
    return f


@functools.lru_cache(maxsize=None)
def _alone(n, P, Np, focused, count_wgs=0):
    """the flagged pf_run of every chunk on its own, computed once per shape and left unchanged"""
    out = []
    for k, (m, sg) in enumerate(_chunks(n, P, focused)):
        f = _new(m, sg, Np, 3 + k, count_wgs=count_wgs)
        assert f.run_path() == "SweepXlmp"
        f.run(); f.finish()
        out.append(_snap(f))
        f.close()
    return out


def _group(n, P, Np, focused, count_wgs=0):
    return [_new(m, sg, Np, 3 + k, count_wgs=count_wgs) for k, (m, sg) in enumerate(_chunks(n, P, focused))]


def _all_same(many, alone):
    for f, g in zip(many, alone):
        _same(_snap(f), g)


def _close(many):
    for f in many:
        f.close()


@pytest.mark.parametrize("n,P,Np,focused", LOCK)
def test_chunks_in_lockstep_equal_their_own_flagged_runs(hiplib, n, P, Np, focused):
    """Four chunks with their own data, lengths and seeds through pf_run_many in calls of 29 rows: every chunk has the bits of its own
    flagged pf_run, counts included (the sums are grouped by workgroup the same way)."""
    alone = _alone(n, P, Np, focused)
    many = _group(n, P, Np, focused)
    try:
        assert ParticleFilter.can_run_many(many)
        assert all(f.run_path(many=True) == "SweepXlmp" for f in many)
        assert len({f.n_segs for f in many}) == len(many)
        assert min(f.n_segs for f in many) >= 40          # the sixteen-slot rings wrap, the every-eighth-step wait is reached
        _lockstep(many, CALL)
        for f in many:
            assert int(f.trace()["resampled"].sum()) >= 3
        assert any(int(np.asarray(f.migrations()["n_events"]).sum()) > 0 for f in many)
        _all_same(many, alone)
    finally:
        _close(many)


def test_one_count_workgroup_per_column_in_lockstep(hiplib):
    """count_wgs = 1 on both sides (Np = 320 has two particle blocks of 256: the default is two workgroups a column)"""
    n, P, Np, focused = HEAD
    alone = _alone(n, P, Np, focused, 1)
    many = _group(n, P, Np, focused, 1)
    try:
        assert ParticleFilter.can_run_many(many)
        _lockstep(many, CALL)
        _all_same(many, alone)
    finally:
        _close(many)


def test_another_chunk_leading(hiplib):
    """the handles in reverse order: another leader (its streams, its table), another blockIdx.y for every chunk"""
    n, P, Np, focused = HEAD
    alone = _alone(n, P, Np, focused)
    many = _group(n, P, Np, focused)
    try:
        _lockstep(many[::-1], CALL)
        _all_same(many, alone)
    finally:
        _close(many)


def test_step_api_and_a_run_alone_between_two_lockstep_calls(hiplib):
    """58 rows of all chunks in lockstep, then five rows of chunk 2 by pf_run and of chunk 3 by single steps (update_segment / count /
    resample: the general kernels, on two of the sixteen slots) while the other two take theirs in lockstep, then the rest together"""
    n, P, Np, focused = HEAD
    alone = _alone(n, P, Np, focused)
    many = _group(n, P, Np, focused)
    try:
        nmax = max(f.n_segs for f in many)
        s = 58
        assert min(f.n_segs for f in many) > s + 5
        ParticleFilter.run_many(many, 0, s)
        many[2].run(s, s + 5)
        for r in range(s, s + 5):
            many[3].update_segment(r); many[3].count(r); many[3].resample(r)
        ParticleFilter.run_many(many[:2], s, s + 5)
        ParticleFilter.run_many(many, s + 5, nmax)
        for f in many:
            f.finish()
        _all_same(many, alone)
    finally:
        _close(many)


# ---------------------------------------------------------------- 4. refusals
def _refused(group, why):
    assert not ParticleFilter.can_run_many(group)
    with pytest.raises(PfError, match=why):
        ParticleFilter.run_many(group)


def test_groups_the_launches_cannot_serve_are_refused(hiplib):
    def made(n, P, seed, **kw):
        base = cases.make_model(n=n, E=6, L=4e4)
        segs = cases.make_segments(base, seed=2, max_seg_len=4000)
        kw.setdefault("mp_rows", True)
        f = ParticleFilter(cases.make_structured(base, P=P, split_epoch=4, mig=1.5), 256, seed=seed, **kw)
        f.init_prior(0.0); f.load_segments(segs)
        return f
    a, b = made(12, 2, 1), made(12, 2, 2)
    others = [made(9, 2, 2), made(12, 4, 2), made(12, 2, 2, mp_rows=False), made(12, 2, 2, mig_cap=64)]
    try:
        assert ParticleFilter.can_run_many([a, b]) and ParticleFilter.can_run_many([b])
        with pytest.raises(PfError, match="twice"):
            ParticleFilter.run_many([a, a])
        _refused([a, others[0]], "pf_run_many: the chunks must share .*haplotypes")         # n = 12 with n = 9
        _refused([others[0], a], "pf_run_many: the chunks must share .*haplotypes")
        _refused([a, others[1]], "pf_run_many: the chunks must share .*populations")        # P = 2 with P = 4
        _refused([a, others[2]], "pf_run_many: .*PF_FLAG_MP_LDS_ROWS -- every chunk")       # flagged with unflagged
        _refused([others[2], a], "pf_run_many: .*PF_FLAG_MP_LDS_ROWS -- every chunk")
        _refused([a, others[3]], "pf_run_many: the chunks must share .*mig_cap")            # two mig_caps
    finally:
        _close([a, b] + others)


# ---------------------------------------------------------------- 5. rings
@pytest.mark.parametrize("log_cap,gen_cap,what", [(16, 4096, "event log ring overflow"), (4096, 20, "generation ledger overflow")])
def test_a_ring_too_small_is_a_reported_error(hiplib, log_cap, gen_cap, what):
    """Lags of 60 000 bases keep more records and generations alive than the ring holds: the run stops with the error, it does not go on
    with other numbers (the extend role runs up to fourteen rows ahead and checks its own writes to the event log, Ctrl::g_safe)."""
    model, segs = _inputs(9, 8, 2, 12, False, L=3.0e5, lag=60000.0)
    g = _flagged(model, segs, 192, 3, log_cap=log_cap, gen_cap=gen_cap)
    try:
        assert g.run_path() == "SweepXlmp"
        with pytest.raises(PfError, match=what):
            g.run(); g.finish()
    finally:
        g.close()


def test_rings_that_wrap_many_times(oracle, hiplib):
    """event log of 64 records a slot, ledger of 32 generations, 256 pieces: each wraps more than ten times and the bits are the oracle's"""
    n, E, P, Np, seed = 9, 8, 2, 192, 21
    model, segs = _inputs(n, E, P, seed, False, L=4.0e5, lag=2500.0)
    g = _flagged(model, segs, Np, seed, log_cap=64, gen_cap=32, piece_cap=256)
    try:
        assert g.run_path() == "SweepXlmp"
        g.run(); g.finish()
        o = _oracle_run(oracle, n, E, P, Np, seed, False, 4.0e5, 2500.0)
        _assert_oracle_parity(o, g)
        assert int(o.trace()["resampled"].sum()) > 10 * 32
        assert g.stats()["records"] / Np > 10 * 64
    finally:
        g.close()


def test_too_many_migration_events_is_the_oracles_error(oracle, hiplib):
    n, E, P, Np, seed = 9, 8, 2, 128, 9
    model, segs = _inputs(n, E, P, seed, False)
    with pytest.raises(RuntimeError, match="too many migration events on one local tree"):
        o = oracle.Oracle(model, Np, ess_fraction=0.5, seed=seed, max_trace_events=8, mig_cap=4)
        o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
    g = _flagged(model, segs, Np, seed, mig_cap=4)
    try:
        assert g.run_path() == "SweepXlmp"
        with pytest.raises(PfError, match="too many migration events on one local tree"):
            g.run(); g.sync()
    finally:
        g.close()


# ---------------------------------------------------------------- 6. bin/smcsmc -mp_rows
def test_binary_mp_rows_chunks_side_by_side(hiplib, built_binary, tmp_path):
    """bin/smcsmc -mp_rows -chunks 3 on two populations of six haplotypes each: the chunks of the rank share the launches of a row, and
    the .out equals, character for character, the table written from the same three chunks through the python binding with
    mp_rows=True (the chunk's window, seed + chunk, the sums in chunk order with three sets of prior pseudo-counts)."""
    from smcsmc_amd import outfile, reduce as reducer, simulate, segments as segmod
    n, L, K, Np = 12, 240000, 3, 160
    base = cases.make_model(n=n, E=8, L=float(L))
    seg = str(tmp_path / "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(L), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=40 + n))
    core = ("-N0 10000 -t %g -r %g %d -I 2 6 6 -eN 0.0 1.0 -ema 0.0 0 2.0 2.0 0 -eN 0.1 1.0 -ema 0.1 0 2.0 2.0 0 "
            "-eN 0.5 1.0 -ema 0.5 0 0 0 0 -ej 0.5 2 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", str(Np), "-seed", "5", "-lag", "50000", "-chunks", str(K), "-ranks", "1"]

    def run(name, extra):
        r = subprocess.run([built_binary] + core + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        return open(tmp_path / (name + ".out")).read(), r.stderr

    text, err = run("rows", ["-mp_rows"])
    assert "%d chunk(s) ran side by side" % K in err

    m = json.loads(subprocess.run([built_binary] + core + ["-nsam", str(n), "-tmax", "4", "-mp_rows", "-dumpmodel"], capture_output=True, text=True).stdout)
    assert m["mp_rows"] is True and m["npop"] == 2
    E = len(m["change_times"])
    mig = np.array(m["mig_rates"]).reshape(E, 2, 2); smig = np.array(m["single_mig"]).reshape(E, 2, 2)
    sizes = np.array(m["pop_sizes"]).reshape(E, 2)
    first = [1 + (L * c) // K for c in range(K + 1)]
    total = None
    for c in range(K):
        length = first[c + 1] - first[c]
        model = dict(change_times=np.array(m["change_times"]), pop_sizes=sizes, lags=np.full(E, 50000.0), nsam=n, loci_length=float(length),
                     mutation_rate=m["mutation_rate"], recombination_rate=m["recombination_rate"], n_pops=2, mig_rates=mig, single_mig=smig,
                     sample_pops=m["sample_pops"])
        S = segmod.Segments(seg, n, length, data_start=first[c], max_segment_length=int(2.0 / (m["recombination_rate"] * 4 * m["N0"])))
        segs = S.pack(model["lags"])
        g = ParticleFilter(model, Np, seed=5 + c, max_trace_events=0, local_recomb=True, mp_rows=True)
        g.init_prior(segs["start"][0]); g.load_segments(segs)
        assert g.run_path() == "SweepXlmp"
        g.run(); g.finish()
        packed = reducer.pack_counts(g.counts())
        g.close()
        total = packed.copy() if total is None else total + packed            # chunk order, as run_chunks sums
    t = reducer.unpack_counts(total, E, 2)
    Kf = float(K)
    end = lambda e: 1e+99 if e == E - 1 else m["change_times"][e + 1]      # noqa: E731
    out = [outfile.HEADER]
    for e in range(E):
        for a in range(2):
            out.append(outfile.format_row(0, e, m["change_times"][e], end(e), "Coal", a, -1, t["coal_opp"][e, a] + Kf,
                                          t["coal_count"][e, a] + Kf / (2.0 * sizes[e, a]), t["coal_weight"][e, a] + Kf))
    ropp = rcount = rweight = 0.0
    for e in range(E):
        ropp += t["rec_opp"][e] + Kf
        rcount += t["rec_count"][e] + Kf * m["recombination_rate"]
        rweight += t["rec_weight"][e] + Kf
    out.append(outfile.format_row(0, -1, 0.0, 1e+99, "Recomb", -1, -1, ropp, rcount, rweight))
    for e in range(E):
        for a in range(2):
            for b in range(2):
                if a != b:
                    out.append(outfile.format_row(0, e, m["change_times"][e], end(e), "Migr", a, b, t["mig_opp"][e, a] + Kf,
                                                  t["mig_count"][e, a, b] + Kf * mig[e, a, b], t["mig_weight"][e, a] + Kf))
    out.append(outfile.format_row(0, -1, 0.0, 1e+99, "Delay", -1, -1, t["delayed_opp"], t["delayed_count"] / Np, t["delayed_opp"]))
    out.append(outfile.format_row(0, -1, 0.0, 1e+99, "Resamp", -1, -1, t["delayed_opp"], t["resample_count"], t["delayed_opp"]))
    out.append(outfile.format_row(0, -1, 0, 1e+99, "LogL", -1, -1, 1.0, t["logl"], 1.0))
    assert "".join(out) == text and "Migr" in text
