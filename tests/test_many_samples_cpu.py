"""More than 16 haplotypes: what the binary refuses before it touches a device (one population only, no -arg, no -apf, at
most 64), and the library's declarations of the wide path.  Runs without a GPU."""
import os
import re
import subprocess

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
