"""More than 16 haplotypes: what the binary refuses before it touches a device (one population only, no -arg, no -apf, at
most 64), and the library's declarations of the wide path.  Runs without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["-Np", "5", "-t", "1", "-r", "1", "100000"]


@pytest.fixture(scope="module")
def binary(built_binary):
    return built_binary


@pytest.mark.parametrize("args,msg", [
    (["-nsam", "65"], "at most 64 haplotypes"),
    (["-nsam", "24", "-I", "2", "12", "12"], "more than 16 haplotypes need one population"),
    (["-nsam", "24", "-arg"], "-arg with more than 16 haplotypes"),
    (["-nsam", "24", "-apf", "1"], "-apf with more than 16 haplotypes"),
])
def test_binary_refuses_what_the_wide_path_does_not_cover(binary, args, msg):
    r = subprocess.run([binary] + BASE + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith("Error: ") and msg in r.stderr, r.stderr


@pytest.mark.parametrize("nsam", ["17", "32", "64"])
def test_binary_accepts_up_to_64_haplotypes(binary, nsam):
    """-dumpmodel parses and prints the model without running the filter"""
    r = subprocess.run([binary] + BASE + ["-nsam", nsam, "-dumpmodel"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert '"nsam": %s' % nsam in r.stdout


def test_header_declares_the_wide_path():
    header = open(os.path.join(ROOT, "include", "smcsmc_pf.h")).read()
    assert re.search(r"#define PF_DEBUG_FORCE_WIDE 2048\b", header)
    bits = [int(v) for v in re.findall(r"#define PF_DEBUG_\w+ (\d+)\b", header)]
    assert len(bits) == len(set(bits)), "two debug switches share a bit"
    from smcsmc_amd import pf
    assert pf.DEBUG_FORCE_WIDE == 2048 and pf.NSAM_MAX_WIDE == 64


REMOVED_DEBUG_BITS = {"SPLIT_ROLES": 64, "COUNT_YOUNG_FIRST": 512, "CU_MASK": 1024, "FLAG_HANDOFF": 8192}


def test_removed_launch_arrangements_are_gone_and_refused_by_name():
    """The switches of the three launch arrangements that lost their A/B are neither declared nor used, and pf_create -- before it
    touches a device -- refuses a debug value that still sets one of their bits, naming the bit."""
    import ctypes as C
    from smcsmc_amd import pf
    sources = [os.path.join(ROOT, "include", "smcsmc_pf.h")]
    for d, _, files in os.walk(os.path.join(ROOT, "smcsmc_amd")):
        sources += [os.path.join(d, f) for f in files if f.endswith((".h", ".hpp", ".hip", ".cpp", ".py", "Makefile"))]
    assert len(sources) > 20
    for path in sources:
        text = open(path, errors="replace").read()
        for name in REMOVED_DEBUG_BITS:
            assert name not in text, "%s still names %s" % (path, name)
    L = pf.load_library()
    model = pf._Model()
    for bit in REMOVED_DEBUG_BITS.values():
        for debug in (bit, bit | pf.DEBUG_NO_COUNT):
            params = pf._Params(np=100, ess_fraction=0.5, seed=1, debug=debug)
            assert L.pf_create(C.byref(model), C.byref(params), 0) is None
            assert "debug bit %d " % bit in pf._err(L) and "removed" in pf._err(L), pf._err(L)


# ---------------------------------------------------------------- the oracle states the same limits as the device path
def test_oracle_accepts_64_haplotypes_with_one_population(oracle):
    import cases
    model = cases.make_model(n=64, E=4, L=1e4)
    o = oracle.Oracle(model, 8, seed=1)
    o.init_prior(0.0)
    p = o.particles()
    assert p["children"].shape == (8, 63, 2) and p["children"].max() == 2 * 64 - 3 and (p["heights"] > 0).all()
    o.close()
    with pytest.raises(RuntimeError, match="nsam out of range"):
        oracle.Oracle(cases.make_model(n=65, E=4, L=1e4), 8, seed=1)


def test_oracle_refuses_what_the_wide_path_does_not_cover(oracle):
    import cases
    from smcsmc_amd import segments as segmod
    model = cases.make_model(n=17, E=4, L=1e4)
    with pytest.raises(RuntimeError, match="more than 16 haplotypes need one population"):
        oracle.Oracle(cases.make_structured(model, P=2, split_epoch=2), 8, seed=1)
    o = oracle.Oracle(model, 8, seed=1)
    with pytest.raises(RuntimeError, match=r"tree recording \(-arg\) takes nsam <= 16"):
        o.enable_tree_recording()
    segs = cases.make_segments(model, seed=1)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"].reshape(-1, 17))]
    with pytest.raises(RuntimeError, match=r"look-ahead \(-apf\) takes nsam <= 16"):
        o.load_lookahead(segmod.pack_lookahead(rows, 17), 1, (np.ones((17, len(segmod.TBL_QUANTILES))), 1.0))
    o.close()
    # all three are accepted at 16
    m16 = cases.make_model(n=16, E=4, L=1e4)
    oracle.Oracle(cases.make_structured(m16, P=2, split_epoch=2), 8, seed=1).close()
    o = oracle.Oracle(m16, 8, seed=1); o.enable_tree_recording(); o.close()
