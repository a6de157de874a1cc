"""Ancient samples (model key sample_times, -eI) with a time above zero: the device against the CPU oracle, bit for bit.

The oracle knows sample times (oracle/smc_oracle.cpp; what licenses it is tests/test_oracle_ancient_cpu.py: the Monte Carlo fixture, the
rates of a run without data, all-zero times), so the bar is the one of test_gpu_structured.py / test_gpu_wide_pops.py: trace, trees, node
populations, canonical migration lists, weights, next_base and log-likelihood bit-identical, the count sums within COUNT_RTOL = 1e-9.  The
recombination opportunity is the one count the two sides form differently -- the oracle writes one rectangle per time slice and epoch with
the lineages present, the device takes the length that does not exist off the whole tree's (k_count_anc, Win::dead) -- so its agreement is
the check on k_count_anc.  The cases are tests/ancient_cases.py; that every one resamples, is moved by its times and meets the edge it is
for is asserted there on the oracle alone.

Which case launches what, every one with a time above zero:

  kernel                                         cases
  k_init_mp<4 + PF_ANC>, k_extend_mp<.., 4 + PF_ANC>   2-2, 4-2, 5-2-root-wait, 6-2-join, 7-3, 8-4, 9-2, 16-2, 12-3
  k_init_mp<8 + PF_ANC>, k_extend_mp<.., 8 + PF_ANC>   6-6, 8-8, 12-5, 16-8
  k_calibrate_mp<4 + PF_ANC>, <8 + PF_ANC>             test_calibration_parity (6, 2) and (6, 6)
  k_count_anc<4, 2>     2-2 (one-node tree, one lineage below the time), 4-2 (two distinct entry times)
  k_count_anc<8, 2>     5-2-root-wait (mp_root_wait across the join), 6-2-join (samples enter where population 1 is moved)
  k_count_anc<8, 4>     7-3, 8-4 (and the narrow variants)
  k_count_anc<16, 2>    9-2, 16-2
  k_count_anc<16, 4>    12-3
  k_count_anc<8, 8>     6-6 (and the wide variants), 8-8
  k_count_anc<16, 8>    12-5, 16-8

Variants on 8-4 and 6-6: a block with two samples missing among unphased sites, -vb event counts (the factor of a migration of the
waiting root included), the 100-bp local recombination map, PF_DEBUG_NO_FUSE."""
import numpy as np
import pytest

import ancient_cases as ac
import oracle_lib
from test_gpu_wide_pops import COUNT_RTOL, NO_FUSE, _assert_counts_close, _assert_state_equal, _assert_trace_equal, _bits

pytestmark = pytest.mark.gpu


def _device(case_id, variant=None):
    from smcsmc_amd import ParticleFilter
    c = ac.by_id(case_id)
    model, segs = ac.inputs(case_id, None if variant == "no-fuse" else variant)
    kw = {}
    if variant == "no-fuse":
        kw["debug"] = NO_FUSE
    if variant == "local_map":
        kw["local_recomb"] = True
    g = ParticleFilter(model, c["Np"], ess_fraction=0.5, seed=c["seed"], max_trace_events=64, **kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    assert g.run_path() == "General" and g.run_path(many=True) is None
    g.run(); g.finish()
    return model, g


def _compare(ref, model, g):
    assert ref["trace"]["resampled"].sum() > 0, "the case must exercise resampling"
    assert max(model["sample_times"]) > 0
    assert _bits([g.logl()])[0] == _bits([ref["logl"]])[0]
    _assert_trace_equal(ref, g)
    _assert_state_equal(ref, g)
    co, cg = ref["counts"], g.counts()
    assert co["rec_opp"].min() >= 0 and co["rec_opp"].sum() > 0
    _assert_counts_close(co, cg)


@pytest.mark.parametrize("case_id", ac.IDS)
def test_ancient_full_sweep_parity(hiplib, case_id):
    model, g = _device(case_id)
    try:
        _compare(ac.oracle_run(case_id), model, g)
    finally:
        g.close()


@pytest.mark.parametrize("case_id", ac.VARIANT_CASES)
@pytest.mark.parametrize("variant", ac.VARIANTS)
def test_ancient_variant_parity(hiplib, case_id, variant):
    model, g = _device(case_id, variant)
    try:
        ref = ac.oracle_run(case_id, None if variant == "no-fuse" else variant)
        _compare(ref, model, g)
        if variant == "local_map":
            # (the rule of test_gpu_many_samples.py for the map: the cumulated differential opportunity, every per-sample row)
            n = model["nsam"]
            lo, lg = ref["local_recomb"], g.local_recomb()
            cum_o, cum_g = np.cumsum(lo["opp_diff"]), np.cumsum(lg["opp_diff"])
            np.testing.assert_allclose(cum_g, cum_o, rtol=1e-7, atol=1e-7 * cum_o.max())
            assert lo["counts"][:n].sum() > 0
            assert lg["counts"].shape == lo["counts"].shape == (n + 2, len(lo["opp_diff"]))
            np.testing.assert_allclose(lg["counts"], lo["counts"], rtol=COUNT_RTOL, atol=1e-12 * max(1.0, lo["counts"].max()))
            assert lg["counts"][:n].sum() == pytest.approx(g.counts()["rec_count"].sum(), rel=COUNT_RTOL)
    finally:
        g.close()


@pytest.mark.parametrize("P", ac.CALIBRATION_POPS)
def test_calibration_parity(hiplib, P):
    """k_calibrate_mp<PW + PF_ANC> with times above zero: the median survival distances and the number of trees used are the oracle's.
    (One batch of 16 384 trees on either side, the least a calibration draws; that the times move the result is asserted on the oracle in
    tests/test_oracle_ancient_cpu.py.)"""
    from smcsmc_amd import pf
    model = ac.calibration_model(P)
    assert model["nsam"] == 6 and model["n_pops"] == P and max(model["sample_times"]) > 0
    dm, dt = pf.median_survival(model, seed=1, min_events=50, max_trees=16384)
    om, ot = oracle_lib.median_survival(model, seed=1, min_events=50, max_trees=16384)
    assert dt == ot == 16384
    assert (_bits(dm) == _bits(om)).all()
