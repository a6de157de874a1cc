"""The device against the model's own statement of the site weight under unphased marks, dephase and ancestral_aware
(tests/mc_model.py, tests/golden/mc_model_emission.json).

The body is tests/mc_model_check.py, the one tests/test_mc_model_emission_cpu.py applies to the oracle: over 32 fixed seeds
log(mean exp(logl)) and the exp(logl)-weighted counts of ParticleFilter equal the brute-force numbers within 4 combined standard errors,
at a combined relative standard error of at most 3 % (log p) and 6 % (a compared cell).  The seeds run as chunks of run_many, eight to a
call; for the first two seeds the log-likelihood also carries the oracle's bits.  Every case lies at least 0.3 in log p from its twin
without the flag, so a kernel that ignored a flag would miss by ten standard errors or more."""
import numpy as np
import pytest

import mc_model_check as chk
import test_mc_model_emission_cpu as cpu

pytestmark = pytest.mark.gpu
gold = cpu.gold


@pytest.mark.parametrize("case,mode", cpu.CHECKS)
def test_the_device_targets_the_model_under_marks_and_flags(hiplib, oracle, gold, case, mode):
    res, logl = chk.device_check(case, mode)
    for seed, dev in zip(chk.SEEDS, logl):
        if seed in chk.BIT_SEEDS:
            ref = chk.oracle_run((case, mode, seed))[0]
            assert np.float64(dev).view(np.uint64) == np.float64(ref).view(np.uint64), (seed, dev, ref)
