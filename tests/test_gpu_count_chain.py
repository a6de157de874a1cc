"""The counting chain of a split step (run_sweep_split, csrc/pf_run.h): the second launch of a row, k_sweep_blc4 on the counting stream, and the
completion signals that pace it against the extend launches through the sixteen-slot ring.

Only the second launches that a wait reads carry a completion signal: one in eight for the ring (SweepFrame::ring_wait, seven steps later) and
the last of the call (SweepFrame::leave).  A wait that met no record of its own step would return at once and let the extend role overwrite a
ring slot the counts still read; that shows as counts, or a ledger, that differ from the one-launch form, and not in every run.  The kernel
itself plans its step without the end of the row before (it has no bookkeeping role) and a count workgroup requests its accumulator when it
starts, not behind its last sum: the one-launch form and k_sweep_blc4q keep the old code and are the comparators.  So, by the
conventions of test_gpu_sweep.py (log-likelihood, trace, resampling parents, particles and counts, bit for bit) and of
test_gpu_pair_handoff.py (the oracle computed once a case and shared):

(i)   the default path against every role of a step in ONE launch (PF_DEBUG_ONE_LAUNCH: no second stream, no ring waits) and against the
      oracle, for both instances of k_sweep_blc4 (four haplotypes and fewer), one count workgroup a column, a second one with one particle and
      several, at ESS fractions where nearly every row runs the ledger items, about half do, and none does; once with 32 epochs;
(ii)  the same sweep in calls of 1 to 41 rows: every ring phase as first row, calls shorter than the first awaited step, a last step that
      is and is not one the ring waits for, and the accumulators continued behind an earlier call's totals;
(iii) a signal on every second launch (PF_DEBUG_SIGNAL_ALL_COUNTS, the arrangement up to round 19): the same bits;
(iv)  chunks in lockstep (pf_run_many), each equal to its own run: two of unequal length, five on the one-wavefront row kernel, a group with
      count_wgs and one with count_workers (k_sweep_blc4q);
(v)   one case three times in one process;
(vi)  an event log too small for the data: the error of the one-launch form.

Rows are 259 (n = 4) and 120 (n = 3): the ring wait fires thirty-two and fifteen times a run.  Each case asserts from the oracle how many rows resample."""
import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError, pf
from test_gpu_sweep import _bits, _run_alone, _same

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 1 << 23          # PF_DEBUG_ONE_LAUNCH
SEED = 5
_ORACLE = {}
_GPU = {}

# rows that resample, from the oracle: (n, E, Np, ess fraction)
RESAMPLING_ROWS = {(4, 10, 65, 0.9): 224, (4, 10, 65, 0.5): 96, (4, 10, 65, 1e-4): 0, (4, 10, 129, 0.9): 232, (4, 10, 129, 0.5): 106, (4, 10, 129, 1e-4): 0,
                   (4, 10, 257, 0.9): 239, (4, 10, 257, 0.5): 109, (4, 10, 257, 1e-4): 0, (4, 10, 1100, 0.9): 242, (4, 10, 1100, 0.5): 119,
                   (4, 10, 1100, 1e-4): 0, (4, 32, 257, 0.5): 109,
                   (3, 10, 65, 0.9): 103, (3, 10, 65, 0.5): 36, (3, 10, 65, 1e-4): 0, (3, 10, 129, 0.9): 107, (3, 10, 129, 0.5): 52, (3, 10, 129, 1e-4): 0,
                   (3, 10, 257, 0.9): 107, (3, 10, 257, 0.5): 52, (3, 10, 257, 1e-4): 0, (3, 10, 1100, 0.9): 110, (3, 10, 1100, 0.5): 54, (3, 10, 1100, 1e-4): 0}
ROWS = {4: 259, 3: 120}


def _case(n, E=10):
    model = cases.make_model(n=n, E=E, L=1.5e5)
    return model, cases.make_segments(model, seed=11, max_seg_len=4000)


def _oracle_run(oracle, n, E, Np, ess):
    """the oracle's run of a case, computed once and shared (read only)"""
    key = (n, E, Np, ess)
    if key not in _ORACLE:
        model, segs = _case(n, E)
        o = oracle.Oracle(model, Np, ess_fraction=ess, seed=SEED)
        o.init_prior(0.0)
        o.run(o.pack_segments(model, segs))
        _ORACLE[key] = dict(trace=o.trace(), events=o.resample_events(), counts=o.counts(), logl=o.logl())
        o.close()
    return _ORACLE[key]


class _Outputs:
    """what _same and its kin read of a filter, taken once: the filter itself is closed (a handle kept for the session would show as
    live device memory in test_gpu_handle_lifecycle.py)"""

    def __init__(self, f, local_recomb):
        self._d = dict(logl=f.logl(), trace=f.trace(), resample_events=f.resample_events(), counts=f.counts(), particles=f.particles(),
                       local_recomb=f.local_recomb() if local_recomb else None)
        for name in self._d:
            setattr(self, name, lambda name=name: self._d[name])


def _single_call(n, Np, ess, **kw):
    """the default path in one call, computed once a case and shared (read only)"""
    key = (n, Np, ess) + tuple(sorted(kw.items()))
    if key not in _GPU:
        model, segs = _case(n)
        f = _run_alone(model, segs, Np, SEED, 0, ess_fraction=ess, **kw)
        assert f.run_path() == "SweepSplit"
        _GPU[key] = _Outputs(f, kw.get("local_recomb", False))
        f.close()
    return _GPU[key]


def _has_power(ref, key, rows):
    resampling = int(ref["trace"]["resampled"].sum())
    assert len(ref["trace"]["T"]) == rows == ROWS[key[0]]
    assert resampling == RESAMPLING_ROWS[key], (key, resampling)
    ess = key[3]
    if ess == 1e-4:
        assert resampling == 0                       # no row runs a ledger item
    elif ess == 0.9:
        assert resampling >= 0.85 * rows             # six rows in seven do
    else:
        assert 0.25 * rows < resampling < 0.5 * rows # runs of rows with and without them


def _equals_oracle(ref, a):
    assert _bits(a.logl()) == _bits(ref["logl"])
    ta = a.trace()
    for k in ("T", "ess", "logl"):
        assert (_bits(ta[k]) == _bits(ref["trace"][k])).all(), k
    assert (ta["resampled"] == ref["trace"]["resampled"]).all()
    (sg, pg), (so, po) = a.resample_events(), ref["events"]
    assert (sg == so).all() and (pg == po).all()
    cg = a.counts()
    for k in ("coal_count", "coal_opp", "rec_count", "rec_opp"):
        np.testing.assert_allclose(cg[k], ref["counts"][k], rtol=1e-9, atol=1e-300, err_msg=k)


def _equals_one_launch(a, b):
    _same(a, b)
    la, lb = a.local_recomb(), b.local_recomb()
    for k in la:                                     # float atomics: the same terms in any order
        np.testing.assert_allclose(la[k], lb[k], rtol=1e-9, atol=1e-9 * max(1e-300, float(np.abs(lb[k]).max())))


@pytest.mark.parametrize("ess", [0.9, 0.5, 1e-4])
@pytest.mark.parametrize("Np", [65, 129, 257, 1100])
@pytest.mark.parametrize("n", [4, 3])
def test_default_equals_one_launch_and_oracle(oracle, hiplib, n, Np, ess):
    model, segs = _case(n)
    ref = _oracle_run(oracle, n, 10, Np, ess)
    _has_power(ref, (n, 10, Np, ess), len(segs["start"]))
    a = _single_call(n, Np, ess, local_recomb=True)
    b = _run_alone(model, segs, Np, SEED, ONE_LAUNCH, ess_fraction=ess, local_recomb=True)
    assert b.run_path() == "Sweep"
    _equals_one_launch(a, b)
    _equals_oracle(ref, a)
    assert float(np.sum(a.counts()["coal_opp"])) > 0.0          # columns moved: the count items had work
    b.close()


def test_thirty_two_epochs(oracle, hiplib):
    """the depth of the headline benchmark: thirty-two epoch columns a row"""
    model, segs = _case(4, 32)
    ref = _oracle_run(oracle, 4, 32, 257, 0.5)
    _has_power(ref, (4, 32, 257, 0.5), len(segs["start"]))
    a = _run_alone(model, segs, 257, SEED, 0, local_recomb=True)
    b = _run_alone(model, segs, 257, SEED, ONE_LAUNCH, local_recomb=True)
    assert a.run_path() == "SweepSplit" and b.run_path() == "Sweep"
    _equals_one_launch(a, b)
    _equals_oracle(ref, a)
    a.close(); b.close()


@pytest.mark.parametrize("rows", [1, 2, 3, 7, 8, 9, 15, 16, 17, 41])
def test_calls_of_several_lengths(hiplib, rows):
    """Calls of `rows` rows are rows + 2 steps: 1 to 5 end before the first awaited step (8), 7 ends on step 8 and 8 on step 9, the first the
    ring waits for seven steps later; an odd length walks the first row of a call through all sixteen ring phases, 16 keeps it on one."""
    model, segs = _case(4)
    a = _single_call(4, 257, 0.5)
    assert int(a.trace()["resampled"].sum()) == RESAMPLING_ROWS[(4, 10, 257, 0.5)]
    b = _run_alone(model, segs, 257, SEED, 0, step=rows)
    _same(a, b)
    b.close()


@pytest.mark.parametrize("step", [None, 41])
def test_a_signal_on_every_second_launch_changes_nothing(hiplib, step):
    model, segs = _case(4)
    a = _single_call(4, 1100, 0.5, local_recomb=True)
    b = _run_alone(model, segs, 1100, SEED, pf.DEBUG_SIGNAL_ALL_COUNTS, step=step, local_recomb=True)
    assert b.run_path() == "SweepSplit"
    _equals_one_launch(a, b)
    b.close()


def _chunks(k, scale):
    model = cases.make_model(n=4, E=10, L=1.5e5)
    out = []
    for j in range(k):
        m = dict(model, loci_length=float(model["loci_length"] * scale(j)))
        out.append((m, cases.make_segments(m, seed=50 + j, max_seg_len=4000)))
    return out


@pytest.mark.parametrize("k,form,kw", [(2, "paired", {}), (5, "single", dict(debug=pf.DEBUG_NO_PAIR)), (3, "paired", dict(count_wgs=3)),
                                      (3, "paired", dict(count_workers=7))], ids=["two-unequal", "five-k_sweep4", "count_wgs", "count_workers"])
def test_chunks_in_lockstep_equal_their_own_runs(hiplib, k, form, kw):
    """(five chunks: the one-wavefront row kernel k_sweep4 beside the shared k_sweep_blc4 -- at this particle count five chunks would still
    have a compute unit per extend workgroup, so the form is asked for by its switch)"""
    chunks = _chunks(k, lambda j: 0.5 + 0.5 * j / max(1, k - 1))
    alone = [_run_alone(m, sg, 1100, 7 + j, 0, local_recomb=True, **{x: v for x, v in kw.items() if x != "debug"}) for j, (m, sg) in enumerate(chunks)]
    many = []
    for j, (m, sg) in enumerate(chunks):
        f = ParticleFilter(m, 1100, seed=7 + j, local_recomb=True, **kw)
        f.init_prior(0.0); f.load_segments(sg)
        many.append(f)
    nmax = max(f.n_segs for f in many)
    assert min(f.n_segs for f in many) < nmax - 16              # a chunk finishes first, more than a ring earlier
    for s0 in range(0, nmax, 101):
        ParticleFilter.run_many(many, s0, min(nmax, s0 + 101))
        assert many[0].row_form() == form
    for f, g in zip(many, alone):
        f.finish()
        assert f.segments_done() == g.segments_done()
        _equals_one_launch(f, g)
    assert sum(int(f.trace()["resampled"].sum()) for f in many) > 10 * k
    for f in many + alone:
        f.close()


def test_three_runs_in_one_process(oracle, hiplib):
    model, segs = _case(4)
    ref = _oracle_run(oracle, 4, 10, 129, 0.9)
    _has_power(ref, (4, 10, 129, 0.9), len(segs["start"]))
    first = _single_call(4, 129, 0.9, local_recomb=True)
    _equals_oracle(ref, first)
    for _ in range(2):
        g = _run_alone(model, segs, 129, SEED, 0, ess_fraction=0.9, local_recomb=True)
        _same(first, g)
        g.close()


def test_log_too_small_is_the_error_of_the_one_launch_form(hiplib):
    model, segs = _case(4)
    said = []
    for debug in (ONE_LAUNCH, 0):
        g = ParticleFilter(model, 257, seed=SEED, log_cap=8, debug=debug)
        g.init_prior(0.0); g.load_segments(segs)
        with pytest.raises(PfError, match="event log ring overflow") as e:
            g.run(); g.finish()
        said.append(str(e.value))
        g.close()
    assert said[0] == said[1]
