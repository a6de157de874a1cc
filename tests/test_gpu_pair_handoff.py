"""The hand-off of the paired row kernel (k_sweep4p, csrc/pf_pair.h) at the speed of plain LDS instructions.

The two roles of a pair talk through words in LDS (ring, pub, con, fin, lkf, lik), ordered by nothing but the order in which one wavefront's DS
instructions execute.  With polls of tens of nanoseconds where they took hundreds, a weight wavefront sees an entry sooner after its count, a tree
wavefront sees a freed ring slot sooner, and the end of the row is handed over sooner: a mistake in that order shows as a run that differs from the
oracle, and not in every run.  So, by the conventions of test_gpu_pair_rows.py (trace, resampling parents, final particles and log-likelihood, bit
for bit with the oracle):

(i)   ring pressure with that file's construction (ten times the recombination rate, rows of 4000 bp against a ring of eight entries), both
      instances of the kernel (four haplotypes and fewer), a second tree wavefront with one particle (Np = 65) and a second workgroup with one
      (129), at ess fractions 0.5, 0.9 -- nearly every row resamples, the weight wavefront comes to the ring late, behind the old slot's work, and
      back-pressure starts with the first entries -- and 1e-4, where no row resamples;
(ii)  the same run three times in one process: a race shows as a run that differs;
(iii) both ways a row's end is handed over: rows that all end at a site (lkf = 2, the likelihood through lik) and rows without data (lkf = 1).

Each case asserts from the oracle that it has the power it is here for (updates per lane and row, rows that resample).  No case waits for a spin
to expire."""
import numpy as np
import pytest

import cases
from test_gpu_pair_rows import _equals_oracle, _run

pytestmark = pytest.mark.gpu

SEED = 9
_ORACLE = {}
# rows that resample, from the oracle: (n, Np, ess fraction)
RESAMPLING_ROWS = {(4, 65, 0.5): 189, (4, 129, 0.5): 209, (4, 129, 0.9): 263, (3, 65, 0.5): 142, (3, 129, 0.5): 151, (3, 129, 0.9): 211}


def _oracle_run(oracle, key, model, segs, Np, ess):
    """the oracle's run of a case with its update count, computed once and shared (read only)"""
    if key not in _ORACLE:
        o = oracle.Oracle(model, Np, ess_fraction=ess, seed=SEED, max_trace_events=64)
        o.init_prior(segs["start"][0])
        o.run(o.pack_segments(model, segs))
        _ORACLE[key] = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), logl=o.logl(), updates=o.stats()["recombinations"])
        o.close()
    return _ORACLE[key]


def _pressure(n):
    model = cases.make_model(n=n, E=10, L=1.5e5, rho=1e-7)
    segs = cases.make_segments(model, seed=24, max_seg_len=4000)
    assert len(segs["start"]) == {4: 264, 3: 212}[n] and segs["length"].max() == 4000.0
    return model, segs


def _updates_per_lane_and_row(ref, Np):
    return ref["updates"] / (Np * len(ref["trace"]["T"]))


@pytest.mark.parametrize("ess", [0.5, 0.9, 1e-4])
@pytest.mark.parametrize("Np", [65, 129])
@pytest.mark.parametrize("n", [4, 3])
def test_ring_pressure(oracle, hiplib, n, Np, ess):
    model, segs = _pressure(n)
    ref = _oracle_run(oracle, ("pressure", n, Np, ess), model, segs, Np, ess)
    rows, resampling = len(ref["trace"]["T"]), int(ref["trace"]["resampled"].sum())
    assert rows == len(segs["start"])
    assert _updates_per_lane_and_row(ref, Np) >= 3.0            # the rows of 4000 bp take several times the ring's eight entries
    if ess == 1e-4:
        assert resampling == 0 and len(ref["events"][0]) == 0
    else:
        if (n, Np, ess) in RESAMPLING_ROWS:
            assert resampling == RESAMPLING_ROWS[(n, Np, ess)]
        if ess == 0.9:
            assert resampling >= rows - 1                       # every row but the last one
        assert len(ref["events"][0]) == 64                      # the trace's cap
    g = _run(model, segs, Np, SEED, ess_fraction=ess)
    _equals_oracle(ref, g, min_resampling=0 if ess == 1e-4 else 3)
    g.close()


def test_three_runs_in_one_process(oracle, hiplib):
    model, segs = _pressure(4)
    ref = _oracle_run(oracle, ("pressure", 4, 129, 0.9), model, segs, 129, 0.9)
    assert int(ref["trace"]["resampled"].sum()) == 263
    for _ in range(3):
        g = _run(model, segs, 129, SEED, ess_fraction=0.9)
        _equals_oracle(ref, g)
        g.close()


def test_rows_that_all_end_at_a_site(oracle, hiplib):
    """without a largest row length every row ends at its site: each hands its likelihood over"""
    model = cases.make_model(n=4, E=10, L=1.5e5, rho=1e-7)
    segs = cases.make_segments(model, seed=24)
    assert len(segs["start"]) > 200 and (segs["state"] == 0).all()
    ref = _oracle_run(oracle, "sites", model, segs, 129, 0.5)
    assert _updates_per_lane_and_row(ref, 129) >= 3.0
    g = _run(model, segs, 129, SEED)
    _equals_oracle(ref, g)
    g.close()


def test_rows_without_site_likelihood(oracle, hiplib):
    """rows without data, as long as the rows above: no row has a site likelihood, and none resamples"""
    model = cases.make_model(n=4, E=10, L=1.5e5, rho=1e-7)
    segs = cases.nodata_segments(model, seglen=4000.0)
    assert (segs["state"] != 0).all()
    ref = _oracle_run(oracle, "nodata", model, segs, 129, 0.5)
    assert _updates_per_lane_and_row(ref, 129) >= 3.0
    assert int(ref["trace"]["resampled"].sum()) == 0
    g = _run(model, segs, 129, SEED)
    _equals_oracle(ref, g, min_resampling=0)
    g.close()
