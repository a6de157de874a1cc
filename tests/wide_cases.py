"""The runs at 17..64 haplotypes on which tests/test_gpu_many_samples.py compares the wide kernels with the oracle, kept here
so that tests/test_oracle_wide_cpu.py can check without a device what those comparisons rely on (every run resamples, the
unphased sites stay enumerable) and so that the oracle's share of their cost can be timed on a CPU.

Sequence lengths are short on purpose: the oracle's cost per update grows with n, an unphased site costs 2^(heterozygous pairs)
site likelihoods per particle on both sides, and n is what these cases are about.  `seed` picks the simulated data set; for the
unphased cases at n = 63 and 64 it was chosen among the first seeds for few heterozygous pairs at the busiest site."""
import numpy as np

import cases

# id, n, Np, kind, E, L, data seed, max_seg_len
PARITY = [
    dict(id="17-plain", n=17, Np=300, kind="plain", E=8, L=1.0e5, seed=67, msl=5000),
    dict(id="24-biased", n=24, Np=256, kind="biased", E=8, L=8.0e4, seed=74, msl=5000),
    dict(id="32-local_map", n=32, Np=200, kind="plain", E=8, L=6.0e4, seed=82, msl=5000, local_map=True),
    dict(id="33-unphased-missing-local_map", n=33, Np=200, kind="unphased", E=8, L=4.0e4, seed=83, msl=2000, local_map=True,
         missing=(10000.0, 20000.0, tuple(range(20, 33)))),
    dict(id="48-guide", n=48, Np=130, kind="guide", E=6, L=6.0e4, seed=98, msl=5000),
    dict(id="63-unphased", n=63, Np=100, kind="unphased", E=8, L=1.2e4, seed=113, msl=1000),
    dict(id="64-plain", n=64, Np=100, kind="plain", E=8, L=6.0e4, seed=114, msl=5000),
    dict(id="64-unphased-local_map", n=64, Np=100, kind="unphased", E=8, L=1.2e4, seed=102, msl=1000, local_map=True),
    dict(id="64-plain-32epochs", n=64, Np=1000, kind="plain", E=32, L=4.0e4, seed=116, msl=5000),
]


def by_id(case_id):
    return [c for c in PARITY if c["id"] == case_id][0]


def inputs(case):
    """(model, packed rows) of a case"""
    n, E = case["n"], case["E"]
    data_model = cases.make_model(n=n, E=E, L=case["L"])
    model = data_model
    if case["kind"] == "biased":
        model = dict(model, bias_heights=[400.0], bias_strengths=[3.0, 1.0], delay_type=0, application_delays=np.full(E, 3000.0))
    if case["kind"] == "guide":
        model = dict(model, guide=cases.guide(model, 9, 2.5, n), application_delays=np.full(E, 3000.0))
    segs = cases.make_segments(data_model, seed=case["seed"], max_seg_len=case["msl"], unphased=case["kind"] == "unphased",
                               missing_block=case.get("missing"))
    return model, segs


def run_oracle(oracle_lib, case, model, segs):
    o = oracle_lib.Oracle(model, case["Np"], seed=case["n"], max_trace_events=64)
    if case.get("local_map"):
        o.enable_local_recomb()
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    return o


def max_unphased_pairs(segs):
    """most pairs (2j, 2j + 1) with code 2 at one site"""
    al = np.asarray(segs["alleles"])
    al = al.reshape(len(segs["start"]), -1)
    return int(((al[:, 0:al.shape[1] - 1:2] == 2).sum(axis=1)).max())
