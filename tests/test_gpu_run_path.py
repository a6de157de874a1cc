"""Which runner takes the rows of a handle (run_path() of csrc/pf_run.h, the table "Which path runs when" of DESIGN.md): asked of freshly
made handles, one case per row of that table, and shown by the launch counters of one tiny run per path.  The bit-identity tests compare
the paths with each other and with the oracle; a handle that silently fell back to the general kernels would pass all of them."""
import functools

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, pf

pytestmark = pytest.mark.gpu

NP, E = 256, 4
PF_RING = 16
FORCE_LDS, NO_FUSE, TWO_LAUNCH, K_PIPE, FORCE_WIDE, ONE_LAUNCH = 1, 2, 8, 16, 2048, 1 << 23


@functools.lru_cache(maxsize=None)
def _inputs(n, P=1, kind="plain"):
    base = cases.make_model(n=n, E=E, L=2e5)
    segs = cases.make_segments(base, seed=40 + n, max_seg_len=2000)
    model = base
    if kind == "focused":
        model = dict(base, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(E, 2500.0), delay_type=0)
    elif kind == "guide":
        model = dict(base, guide=cases.guide(base, 5, 2.5, n), application_delays=np.full(E, 3000.0))
    if P > 1:
        model = cases.make_structured(model, P=P, split_epoch=E - 1, mig=2.0)
    return base, model, segs


def _lookahead_rows(segs):
    return [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]


@functools.lru_cache(maxsize=None)
def _lookahead(n):
    """as tests/test_gpu_parity.py loads one (level 2); the quantile table from few trees: only its shape matters here"""
    from smcsmc_amd import segments as segmod
    base, _, segs = _inputs(n)
    return segmod.pack_lookahead(_lookahead_rows(segs), n), pf.terminal_branch_quantiles(base, seed=1, n_trees=2000)


def _new(n, P=1, kind="plain", Np=NP, apf=False, **kw):
    _, model, segs = _inputs(n, P, kind)
    f = ParticleFilter(model, Np, seed=5, **kw)
    f.init_prior(0.0); f.load_segments(segs)
    if apf:
        f.load_lookahead(*((_lookahead(n)[0], 2, _lookahead(n)[1])))
    return f


# (id, handle, run(), run_many()): the rows of the table, top to bottom
TABLE = [
    ("n2", dict(n=2), "SweepSplit", "SweepSplit"),
    ("n4", dict(n=4), "SweepSplit", "SweepSplit"),
    ("n2-one-launch", dict(n=2, debug=ONE_LAUNCH), "Sweep", "Sweep"),
    ("n4-one-launch", dict(n=4, debug=ONE_LAUNCH), "Sweep", "Sweep"),
    ("n4-focused", dict(n=4, kind="focused"), "Sweep", "Sweep"),
    ("n2-guide", dict(n=2, kind="guide"), "Sweep", "Sweep"),
    ("n4-arg", dict(n=4, record_trees=True, gen_cap=64, log_cap=64), "Sweep", "Sweep"),
    ("n5", dict(n=5), "Sweep", "Sweep"),
    ("n8", dict(n=8), "Sweep", "Sweep"),
    ("n4-k-pipe", dict(n=4, debug=K_PIPE), "KPipe", "Sweep"),
    ("n8-k-pipe", dict(n=8, debug=K_PIPE), "KPipe", "Sweep"),
    ("n4-two-launch", dict(n=4, debug=TWO_LAUNCH), "TwoLaunch", None),
    ("n8-two-launch", dict(n=8, debug=TWO_LAUNCH), "TwoLaunch", None),
    ("n2-131073-particles", dict(n=2, Np=131073, gen_cap=32, log_cap=32), "TwoLaunch", None),
    ("n4-no-fuse", dict(n=4, debug=NO_FUSE), "General", None),
    ("n8-force-lds", dict(n=8, debug=FORCE_LDS), "General", None),
    ("n5-force-wide", dict(n=5, debug=FORCE_WIDE), "General", None),
    ("n4-apf", dict(n=4, apf=True), "General", None),
    ("n8-apf", dict(n=8, apf=True), "General", None),
    ("n9", dict(n=9), "General", "SweepXl"),
    ("n16", dict(n=16), "General", "SweepXl"),
    ("n9-apf", dict(n=9, apf=True), "General", None),
    ("n16-arg", dict(n=16, record_trees=True, gen_cap=64, log_cap=64), "General", None),
    ("n9-short-generation-ring", dict(n=9, gen_cap=PF_RING + 3), "General", None),
    ("n9-generation-ring", dict(n=9, gen_cap=PF_RING + 4), "General", "SweepXl"),
    ("n16-no-fuse", dict(n=16, debug=NO_FUSE), "General", None),
    ("n9-two-launch", dict(n=9, debug=TWO_LAUNCH), "General", None),
    ("n17", dict(n=17), "General", None),
    ("P2-n2", dict(n=2, P=2), "SweepXmp", "SweepXmp"),
    ("P2-n8", dict(n=8, P=2), "SweepXmp", "SweepXmp"),
    ("P4-n2", dict(n=2, P=4), "SweepXmp", "SweepXmp"),
    ("P4-n8", dict(n=8, P=4), "SweepXmp", "SweepXmp"),
    ("P2-n8-focused", dict(n=8, P=2, kind="focused"), "SweepXmp", "SweepXmp"),
    ("P2-n8-arg", dict(n=8, P=2, record_trees=True, gen_cap=64, log_cap=64), "General", None),
    ("P2-n2-force-lds", dict(n=2, P=2, debug=FORCE_LDS), "General", None),
    ("P4-n8-no-fuse", dict(n=8, P=4, debug=NO_FUSE), "General", None),
    ("P2-n8-k-pipe", dict(n=8, P=2, debug=K_PIPE), "General", None),
    ("P4-n2-apf", dict(n=2, P=4, apf=True), "General", None),
    ("P2-n9", dict(n=9, P=2), "General", None),
]


@pytest.mark.parametrize("kw,one,many", [pytest.param(*row[1:], id=row[0]) for row in TABLE])
def test_run_path_of_a_handle(hiplib, kw, one, many):
    f = _new(**kw)
    try:
        assert f.run_path() == one
        assert f.run_path(many=True) == many
        # refused exactly where pf_can_run_many says so
        assert ParticleFilter.can_run_many([f]) == (many is not None)
    finally:
        f.close()


@pytest.mark.parametrize("kw,before", [(dict(n=4), "SweepSplit"), (dict(n=8), "Sweep"), (dict(n=4, P=2), "SweepXmp")],
                         ids=["n4", "n8", "P2-n4"])
def test_a_look_ahead_moves_the_handle_to_the_general_kernels(hiplib, kw, before):
    f = _new(**kw)
    try:
        assert f.run_path() == before and f.run_path(many=True) == before
        n = kw["n"]
        f.load_lookahead(_lookahead(n)[0], 2, _lookahead(n)[1])
        assert f.run_path() == "General" and f.run_path(many=True) is None
        assert not ParticleFilter.can_run_many([f])
        f.load_lookahead(_lookahead(n)[0], 0, _lookahead(n)[1])          # level 0 switches it off again
        assert f.run_path() == before
    finally:
        f.close()


# ---------------------------------------------------------------- the paths really are the ones named
ROWS = 40
ESS = 0.9           # high enough that nearly every one of the forty rows resamples


def tiny_run(kw, many):
    """forty rows of one handle; what the launch counters (timing on: every row between a pair of events) and the handle say afterwards"""
    f = _new(ess_fraction=ESS, **kw)
    try:
        f.set_timing(1)
        if many:
            ParticleFilter.run_many([f], 0, ROWS)
        else:
            f.run(0, ROWS)
        launches = {k: v[1] for k, v in f.kernel_times().items()}
        done = f.segments_done()
        resampled = int(np.asarray(f.trace()["resampled"])[:ROWS].sum())
        return dict(launches, done=done, resampled=resampled)
    finally:
        f.close()


# Expected numbers: a run of the parent commit 84a2909 on the same inputs (integers: no tolerance).  The counters are those of
# pf_get_kernel_time: launches of the extend class (rows), decide, count and resample.
TINY = [
    # run_sweep_split: forty-two steps of k_sweep4 + k_sweep_blc4 (forty rows and two flush steps, which are not counted as rows);
    # the bookkeeping, ledger and count roles ride in those launches: no decide, count or resample launch
    ("SweepSplit", dict(n=4), False, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=40)),
    # run_sweep: forty-two k_sweep launches, every role inside
    ("Sweep", dict(n=8), False, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=37)),
    ("Sweep", dict(n=4, debug=K_PIPE), True, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=40)),
    # run_pipeline: forty k_pipe launches and two flush launches (taken off the row count one by one)
    ("KPipe", dict(n=4, debug=K_PIPE), False, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=40)),
    # run_single_stream: per row k_row + k_decide_ledger; the last row is flushed by k_resample and k_ledger
    # (and k_count, had a count window moved within these forty rows)
    ("TwoLaunch", dict(n=4, debug=TWO_LAUNCH), False, dict(extend=40, decide=40, count=0, resample=1, done=40, resampled=40)),
    # run_sweep_x: forty-two steps of k_sweep_xmp + k_sweep_blc
    ("SweepXmp", dict(n=4, P=2), False, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=40)),
    # run_sweep_x through pf_run_many: forty-two steps of k_sweep_xl + k_sweep_blc
    ("SweepXl", dict(n=9), True, dict(extend=40, decide=0, count=0, resample=0, done=40, resampled=36)),
    # the general kernels, for contrast: k_extend, k_decide, k_resample per row, k_count on the nineteen rows whose windows moved
    ("General", dict(n=9), False, dict(extend=40, decide=40, count=19, resample=40, done=40, resampled=36)),
]


@pytest.mark.parametrize("path,kw,many,expect", TINY, ids=["%s-%s" % (t[0], "many" if t[2] else "one") for t in TINY])
def test_the_named_path_is_the_one_that_runs(hiplib, path, kw, many, expect):
    f = _new(**kw)
    try:
        assert f.run_path(many=many) == path
    finally:
        f.close()
    got = tiny_run(kw, many)
    assert got["resampled"] >= 3
    assert got == expect
