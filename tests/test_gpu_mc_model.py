"""The device path against the independent Monte Carlo statement of the model (tests/mc_model.py, tests/golden/mc_model.json).

The body is tests/mc_model_check.py, the one tests/test_mc_model_cpu.py applies to the oracle: over 32 fixed seeds
log(mean exp(logl)) and the exp(logl)-weighted counts of ParticleFilter equal the brute-force numbers within 4 combined
standard errors, at a combined relative standard error of at most 3 % (log p) and 6 % (a compared cell) -- for three and
four samples in one population (the headline kernel's shape), two and four samples in two populations with symmetric and
one-way migration and a join, without and with resampling, with focused sampling (both delay types), a guide and the
look-ahead.  The seeds run as chunks of run_many calls where the shape allows, so the lockstep kernels stand under the same
check; for two seeds per case and mode the log-likelihood carries the oracle's bits.
"""
import numpy as np
import pytest

import mc_model_check as chk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", list(chk.MODES))
@pytest.mark.parametrize("case", chk.CASES)
def test_the_device_targets_the_model(hiplib, oracle, case, mode):
    res, logl = chk.device_check(case, mode)
    for seed, dev in zip(chk.SEEDS, logl):
        if seed in chk.BIT_SEEDS:
            ref = chk.oracle_run((case, mode, seed))[0]
            assert np.float64(dev).view(np.uint64) == np.float64(ref).view(np.uint64), (seed, dev, ref)
