"""Who frees device memory: every handle, whatever stage its creation reached, and every entry point without a handle, whatever it
returned, give back what they took.  Read off the library's own count of the bytes its owners hold (pf_test_live_bytes), which is 0 when
no handle is open -- the shared device's free memory says nothing about one process.  Np = 256, E = 4: the shapes of test_gpu_run_path."""
import gc

import numpy as np
import pytest

from smcsmc_amd import ParticleFilter, pf
from test_gpu_run_path import E, NP, _inputs, _new

pytestmark = pytest.mark.gpu

ROWS = 8


def _live():
    gc.collect()
    return pf.live_bytes()


def _bits(x):
    return np.float64(x).view(np.uint64)


def _logl_of_eight_rows():
    f = _new(n=4)
    try:
        f.run(0, ROWS)
        return _bits(f.logl())
    finally:
        f.close()


REFUSED = [
    ("mig-cap", lambda: (_inputs(4, 2)[1], dict(mig_cap=5000)), "pf_create: mig_cap out of range"),
    ("event-count", lambda: (dict(_inputs(4)[1], vb_coal_counts=[1.0, 1.0, 0.0, 1.0]), {}), "pf_create: variational-Bayes event counts must be positive"),
    ("sample-pops", lambda: (dict(_inputs(4, 2)[1], sample_pops=[0, 1, 2, 0]), {}), "sample population out of range"),
]


@pytest.mark.parametrize("inputs,text", [pytest.param(*r[1:], id=r[0]) for r in REFUSED])
def test_a_refused_creation_leaves_nothing_behind(hiplib, inputs, text):
    assert _live() == 0
    before = _logl_of_eight_rows()
    model, kw = inputs()
    for _ in range(3):
        with pytest.raises(pf.PfError) as e:
            ParticleFilter(model, NP, seed=5, **kw)
        assert str(e.value) == text
        assert _live() == 0
    assert _logl_of_eight_rows() == before
    assert _live() == 0


def _partial_migration():
    sm = np.zeros((E, 2, 2))
    sm[E - 1, 1, 0] = 0.5
    return dict(_inputs(4, 2)[1], single_mig=sm)


@pytest.mark.parametrize("call", [lambda m: pf.terminal_branch_quantiles(m, seed=1, n_trees=2000), lambda m: pf.median_survival(m, min_events=1, max_trees=1)],
                         ids=["terminal_branch_quantiles", "median_survival"])
def test_an_input_error_of_an_entry_point_without_a_handle_leaves_nothing_behind(hiplib, call):
    assert _live() == 0
    with pytest.raises(pf.PfError, match=r"^partial single migration events \(-es/-eps style\) are not supported$"):
        call(_partial_migration())
    assert _live() == 0


def _cycle(kw):
    """create, load, prior, eight rows, the counts (and the tree dump of a recording handle); the open filter"""
    f = _new(**kw)
    f.run(0, ROWS)
    f.counts()
    if kw.get("record_trees"):
        f.finish()
        assert len(f.sample_tree_events(pops=kw.get("P", 1) > 1)[1]) > 0
    return f


SHAPES = [("n4", dict(n=4)), ("n4-arg", dict(n=4, record_trees=True, gen_cap=64, log_cap=64)),
          ("P2-n4-arg", dict(n=4, P=2, record_trees=True, gen_cap=64, log_cap=64))]


@pytest.mark.parametrize("kw", [pytest.param(s[1], id=s[0]) for s in SHAPES])
def test_a_life_cycle_gives_back_what_it_took(hiplib, kw):
    assert _live() == 0
    f1 = _cycle(kw)
    try:
        one = _live()
        assert one > 0
        f2 = _cycle(kw)
        try:
            assert _live() == 2 * one              # two handles of one shape hold the same
        finally:
            f2.close()
        assert _live() == one
    finally:
        f1.close()
    assert _live() == 0
    base, model, _ = _inputs(kw["n"], kw.get("P", 1))
    for call in (lambda: pf.simulate_sites(model, seed=2, nchunks=2), lambda: pf.median_survival(model, min_events=1, max_trees=1),
                 lambda: pf.terminal_branch_quantiles(model, seed=1, n_trees=2000), lambda: pf.device_math(np.linspace(0.1, 2.0, 100))):
        call()
        assert _live() == 0


def test_a_sweep_that_grows_its_chunk_table(hiplib):
    assert _live() == 0
    fs = [_new(n=4) for _ in range(3)]
    try:
        for f in fs:
            ParticleFilter.run_many([f], 0, 4)     # a table of one chunk for every leader
        held = _live()
        ParticleFilter.run_many(fs, 4, ROWS)       # the first leads three: its table is let go and made again, larger
        assert _live() > held
        for f in fs:
            f.sync()
            assert f.segments_done() == ROWS
    finally:
        for f in fs:
            f.close()
    assert _live() == 0
