"""Ancient samples (pf_model.sample_times, PF_MODEL_SAMPLE_TIMES), without a device: what pf_create decides for such a model (pf.plan ->
pf_test_plan), everything it and the tools refuse, by its message, and the kernels the built library carries for it."""
import os
import sys
import tempfile

import numpy as np
import pytest

import cases
from smcsmc_amd import pf
from smcsmc_amd.pf import PfError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE_LDS, NO_FUSE = 1, 2


@pytest.fixture(scope="module", autouse=True)
def lib():
    from smcsmc_amd import build
    build.build_lib()
    return pf.load_library()


def _model(n, P, times=None, E=8):
    m = cases.make_structured(cases.make_model(n=n, E=E, L=1e5), P=P, split_epoch=max(E - 3, 1), mig=1.0) if P > 1 else cases.make_model(n=n, E=E, L=1e5)
    ct = m["change_times"]
    if times is None:                                  # the later half of the samples enters at the start of epoch 2
        times = [0.0] * (n - n // 2) + [float(ct[2])] * (n // 2)
    m["sample_times"] = times
    return m


@pytest.mark.parametrize("kw", [dict(), dict(mp_rows=True), dict(debug=FORCE_LDS), dict(debug=NO_FUSE)], ids=["plain", "mp-rows", "force-lds", "no-fuse"])
@pytest.mark.parametrize("n", [2, 4, 8, 9, 16])
@pytest.mark.parametrize("P", [2, 4, 6, 8])
def test_sample_times_get_no_rings_and_the_times_behind_the_lds_of_the_tree(P, n, kw):
    pl = pf.plan(_model(n, P), 256, seed=5, **kw)
    assert pl["rings"] is None and pl["nslots"] == 2 and pl["smem_pipe"] == 0 and not pl["draw_table"] and pl["workers"] == 0
    plain = dict(_model(n, P))
    del plain["sample_times"]
    base = pf.plan(plain, 256, seed=5, **kw)
    assert pl["smem"] == base["smem"] + 8 * n
    assert {k: v for k, v in pl.items() if k not in ("rings", "nslots", "smem", "smem_pipe")} == \
           {k: v for k, v in base.items() if k not in ("rings", "nslots", "smem", "smem_pipe")}


def test_all_zero_times_are_a_model_with_sample_times():
    pl = pf.plan(_model(8, 2, times=[0.0] * 8), 256, seed=5)
    assert pl["rings"] is None                          # (without the times: the rings of the row pipeline)
    plain = dict(_model(8, 2)); del plain["sample_times"]
    assert pf.plan(plain, 256, seed=5)["rings"] == "Xmp"


def test_the_pointer_is_not_read_without_the_bit():
    """a caller whose struct ends before sample_times: whatever lies there -- here an address that cannot be read -- is left alone"""
    import ctypes as C

    def poison(m, p):
        assert m.flags & pf.MODEL_SAMPLE_TIMES
        m.flags &= ~pf.MODEL_SAMPLE_TIMES
        m.sample_times = C.cast(C.c_void_p(8), C.POINTER(C.c_double))
    plain = dict(_model(8, 2)); del plain["sample_times"]
    assert pf.plan(_model(8, 2), 256, seed=5, tweak=poison) == pf.plan(plain, 256, seed=5)

    def null_with_bit(m, p):
        m.sample_times = None
    assert pf.plan(_model(8, 2), 256, seed=5, tweak=null_with_bit) == pf.plan(plain, 256, seed=5)      # NULL: no sample times


def test_refusals_of_the_times_themselves():
    ct = cases.make_model(n=4, E=8)["change_times"]
    with pytest.raises(PfError, match=r"pf_create: sample time .* of sample 2 is not an entry of change_times"):
        pf.plan(_model(4, 2, times=[0.0, 0.0, 0.5 * (ct[1] + ct[2]), float(ct[2])]), 256)
    with pytest.raises(PfError, match="pf_create: the smallest sample time must be 0"):
        pf.plan(_model(4, 2, times=[float(ct[1])] * 2 + [float(ct[2])] * 2), 256)
    with pytest.raises(PfError, match="pf_create: sample times must ascend with the sample index"):
        pf.plan(_model(4, 2, times=[0.0, float(ct[2]), 0.0, float(ct[2])]), 256)
    with pytest.raises(PfError, match="sample_times needs one entry per sample"):
        pf.plan(_model(4, 2, times=[0.0, 0.0, 0.0]), 256)


def test_refusals_of_what_does_not_run_with_sample_times():
    E = 8
    with pytest.raises(PfError, match="pf_create: sample times .* need a structured model: the one-population kernels count lineages by rank"):
        pf.plan(_model(4, 1), 256)
    with pytest.raises(PfError, match=r"pf_create: tree recording \(-arg\) is not supported with sample times"):
        pf.plan(_model(4, 2), 256, record_trees=True, gen_cap=64, log_cap=64)
    with pytest.raises(PfError, match=r"pf_create: focused sampling \(bias_heights\) is not supported with sample times"):
        pf.plan(dict(_model(4, 2), bias_heights=[400.0], bias_strengths=[5.0, 1.0], application_delays=np.full(E, 1000.0)), 256)
    with pytest.raises(PfError, match="pf_create: a recombination guide is not supported with sample times"):
        m = _model(4, 2)
        pf.plan(dict(m, guide=cases.guide(m, 3, 2.0, 7), application_delays=np.full(E, 1000.0)), 256)


def test_tools_refuse_before_they_ask_for_a_device():
    """pf_simulate_sites and pf_terminal_branch_quantiles say so by name (pf_load_lookahead and pf_run_many need a handle: test_gpu_ancient.py);
    pf_median_survival takes the model and refuses what pf_create refuses about the times"""
    with pytest.raises(PfError, match="pf_simulate_sites: the site simulator is not supported with sample times"):
        pf.simulate_sites(_model(4, 2), seed=1, nchunks=1, max_sites=100)
    with pytest.raises(PfError, match="pf_terminal_branch_quantiles: not supported with sample times"):
        pf.terminal_branch_quantiles(_model(4, 2), seed=1, n_trees=100)
    with pytest.raises(PfError, match="pf_median_survival: the smallest sample time must be 0"):
        ct = cases.make_model(n=4, E=8)["change_times"]
        pf.median_survival(_model(4, 2, times=[float(ct[1])] * 4), seed=1, min_events=10, max_trees=100)
    with pytest.raises(PfError, match="pf_median_survival: sample times .* need a structured model"):
        pf.median_survival(_model(4, 1), seed=1, min_events=10, max_trees=100)


def _all_kernels(lib_path):
    """kernel_meta.kernels() of every offload bundle of the library"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_meta
    b = open(lib_path, "rb").read()
    out = {}
    i = b.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:
        with tempfile.NamedTemporaryFile(suffix=".bundle") as t:
            t.write(b[i:]); t.flush()
            out.update(kernel_meta.kernels(t.name))
        i = b.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 1)
    return out


def test_the_library_carries_the_instances_without_scratch_and_at_the_occupancy_of_their_models():
    """every instance for sample times next to the instance it was made from: no scratch, and no fewer wavefronts on a SIMD -- 512 registers
    (VGPR + AGPR, in blocks of eight) shared by the wavefronts, and for the count instance the LDS of its workgroup"""
    from smcsmc_amd import build
    meta = _all_kernels(build.build_lib())

    def waves(m):
        regs = (m["vgpr"] + m["agpr"] + 7) // 8 * 8
        return min(8, 512 // regs)
    pairs = []
    for pw in (4, 8):             # (the switch rides in the population width: PW + PF_ANC = PW + 16)
        pairs += [("_Z9k_init_mpILi%dEEv5KArgsd" % (pw + 16), "_Z9k_init_mpILi%dEEv5KArgsd" % pw),
                  ("_Z11k_extend_mpILb0ELb0ELi%dEEv5KArgsx" % (pw + 16), "_Z11k_extend_mpILb0ELb0ELi%dEEv5KArgsx" % pw),
                  ("_Z14k_calibrate_mpILi%dEEv5KArgsyxxPiPdS1_" % (pw + 16), "_Z14k_calibrate_mpILi%dEEv5KArgsyxxPiPdS1_" % pw)]
    for nm, P in ((4, 2), (8, 2), (16, 2), (8, 4), (16, 4), (8, 8), (16, 8)):
        pairs.append(("_Z11k_count_ancILi%dELi%dEEv5KArgsi7Windows" % (nm, P), "_Z7k_countILi%dELi%dEEv5KArgsi7Windows" % (nm, P)))
    for new, old in pairs:
        assert new in meta and old in meta, (new, old, sorted(k for k in meta if "_anc" in k or "Li20E" in k or "Li24E" in k))
        a, b = meta[new], meta[old]
        print("%-60s vgpr %3d agpr %2d lds %5d scratch %d   (%s: vgpr %3d agpr %2d lds %5d)" %
              (new, a["vgpr"], a["agpr"], a["lds"], a["scratch"], old, b["vgpr"], b["agpr"], b["lds"]))
        assert a["scratch"] == 0 and b["scratch"] == 0, (new, a)
        assert waves(a) >= waves(b), (new, a, b)
        assert a["lds"] <= b["lds"], (new, a, b)


def _binary(*args):
    import subprocess
    return subprocess.run([os.path.join(ROOT, "bin", "smcsmc")] + [str(a) for a in args], capture_output=True, text=True)


def test_binary_reads_ancient_samples():
    """-eI t n_1 .. n_P: t in units of 4 N0 opens a change point of its own, the samples follow those of -I in column order -- also where -eI
    stands in front of -I --, -nsam is the sum of the -I and -eI counts, -dumpmodel prints the times; the -eI groups keep the order of the
    command line, so a later time in front of an earlier one is refused by name (the library wants ascending times)"""
    import json
    L = 100000
    head = ["-N0", 10000, "-t", 4e4 * 2.5e-8 * L, "-r", 4e4 * 1e-8 * L, L]
    rest = ["-eN", 0, 1.0, "-eM", 0, 2.0, "-eN", 0.5, 1.0, "-ej", 0.5, 2, 1, "-tmax", 4, "-dumpmodel"]
    r = _binary(*head, "-I", 2, 2, 1, "-eI", 0.05, 0, 1, "-eI", 0.2, 1, 1, *rest, "-nsam", 6)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout)
    assert m["change_times"] == [0, 2000, 8000, 20000]                 # 0.05 and 0.2 opened epochs that no other flag names
    assert m["sample_pops"] == [0, 0, 1, 1, 0, 1] and m["sample_times"] == [0, 0, 0, 2000, 8000, 8000]
    assert np.allclose(np.array(m["pop_sizes"]), 1e4) and np.allclose(np.array(m["mig_rates"])[:3, 1], 2.0 / 4e4)     # the new epochs inherit
    r = _binary(*head, "-eI", 0.05, 0, 1, "-I", 2, 2, 1, *rest, "-nsam", 4)
    assert r.returncode == 0 and json.loads(r.stdout)["sample_times"] == [0, 0, 0, 2000]
    r = _binary(*head, "-I", 2, 2, 1, "-eI", 0.2, 1, 1, "-eI", 0.05, 0, 1, *rest, "-nsam", 6)
    assert r.returncode != 0 and "Not supported by this build: -eI times that do not ascend in the order of the command line" in r.stderr + r.stdout
    r = _binary(*head, "-I", 2, 2, 1, *rest, "-nsam", 3)
    assert r.returncode == 0 and json.loads(r.stdout)["sample_times"] == []                                            # no -eI: no times
    r = _binary(*head, "-I", 2, 2, 1, "-eI", 0.05, 0, 1, *rest, "-nsam", 3)
    assert r.returncode != 0 and "Sample sizes in -I and -eI do not add up to -nsam" in r.stderr + r.stdout
    r = _binary(*head, "-I", 2, 2, 1, *rest, "-nsam", 4)
    assert r.returncode != 0 and "Sample sizes in -I do not add up to -nsam" in r.stderr + r.stdout
    r = _binary(*head, "-I", 2, 2, 1, "-eI", 0.05, 0, *rest, "-nsam", 4)
    assert r.returncode != 0                                                                                            # a count short
    for extra, what in ((["-arg"], "-arg with ancient samples"), (["-apf", 2], "-apf with ancient samples"), (["-mp_rows"], "-mp_rows"),
                        (["-bias_heights", 400, "-bias_strengths", 5, 1], "-bias_heights with ancient samples"), (["-guide", "none.txt"], "-guide with ancient samples")):
        r = _binary(*head, "-I", 2, 2, 1, "-eI", 0.05, 0, 1, *rest, "-nsam", 4, *extra)
        assert r.returncode != 0 and "Not supported by this build" in r.stderr + r.stdout and what in r.stderr + r.stdout, (extra, r.stderr)
    r = _binary(*head, "-eI", 0.05, 1, "-eN", 0, 1.0, "-tmax", 4, "-dumpmodel", "-nsam", 1)
    assert r.returncode != 0


def test_em_model_carries_the_sample_times():
    from smcsmc_amd import em
    m = em.PopulationModel(num_samples=4, num_populations=2, change_points=(0.0, 0.05, 0.5), population_sizes=((1, 1), (1, 1), (1, 1)),
                           sample_populations=[1, 2, 1, 2], sample_times=[0, 0, 0.05, 0.05], migration_commands=[None, None, "-ej 0.5 2 1"])
    assert " -I 2 1 1 -eI 0.05 1 1 " in m.core_command_line()
    d = m.device_model(lags=np.full(3, 1e5))
    assert d["sample_times"] == [0.0, 0.0, 2000.0, 2000.0] and d["sample_pops"] == [0, 1, 0, 1]
    assert pf.plan(d, 256)["rings"] is None
    plain = em.PopulationModel(num_samples=4, num_populations=2, change_points=(0.0, 0.05), population_sizes=((1, 1), (1, 1)), sample_populations=[1, 1, 2, 2])
    assert " -I 2 2 2 " in plain.core_command_line() and "-eI" not in plain.core_command_line() and "sample_times" not in plain.device_model()
