"""The hand-off words of the paired row kernel (k_sweep4p, csrc/pf_pair.h) are LDS instructions, checked in the code object the library is linked from.

Through a generic pointer to the __shared__ PairLds every access of a hand-off word compiled to a flat instruction at system scope behind a wait for
all of the wavefront's requests -- 25 of them per instance, several on every pass of the update loop -- where the design says ds_read / ds_write.  The
address space stands in the type of the pointer now (pair_word); this test keeps the flat instructions from coming back unseen: it takes the gfx950
code object out of the built pf_hip object, disassembles the two instances of the kernel and asserts that none of their instructions has a mnemonic
that starts with flat_, and that each has a ds_write_b64 (a ring entry) and an s_sleep (a spin), which shows that the right symbols were found.

No GPU is needed: hipcc cross-compiles.  The tools are the ones beside hipcc's clang; without them the test skips."""
import os
import re
import shutil
import subprocess

import pytest

from smcsmc_amd import build

KERNELS = ("_Z9k_sweep4pILb1EEvPK10SweepChunkxi", "_Z9k_sweep4pILb0EEvPK10SweepChunkxi")      # k_sweep4p<true>, k_sweep4p<false>
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tools():
    hipcc = os.path.realpath(build._hipcc())
    root = os.path.dirname(os.path.dirname(hipcc))
    found = {}
    for name in ("clang-offload-bundler", "llvm-objdump", "llvm-objcopy"):
        for d in (os.path.dirname(hipcc), os.path.join(root, "lib", "llvm", "bin"), os.path.join(root, "llvm", "bin")):
            if os.path.exists(os.path.join(d, name)):
                found[name] = os.path.join(d, name)
                break
        else:
            found[name] = shutil.which(name)
        if not found[name]:
            pytest.skip(name + " not found beside hipcc: the code object cannot be disassembled")
    return found


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """mnemonics of the two instances, from the object file build_lib() links the library from"""
    tools = _tools()
    build.build_lib()
    obj = os.path.join(build.CSRC, "build", "pf_hip.o")
    assert os.path.exists(obj), "build_lib() left no pf_hip object"
    tmp = tmp_path_factory.mktemp("pair_isa")
    fat, co = str(tmp / "pf_hip.hipfb"), str(tmp / "pf_hip.co")
    subprocess.check_call([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp / "copy.o")])
    subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co])
    out = {}
    for k in KERNELS:
        text = subprocess.check_output([tools["llvm-objdump"], "-d", "--no-show-raw-insn", "--disassemble-symbols=" + k, co], text=True)
        out[k] = [m.group(1) for m in (re.match(r"^\s+([a-z][a-z0-9_]+)\b", ln) for ln in text.splitlines()) if m]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_flat_instruction_in_the_paired_kernel(listings, kernel):
    ins = listings[kernel]
    assert len(ins) > 5000, "the kernel was not found in the code object"
    assert "ds_write_b64" in ins and "s_sleep" in ins, "not the paired kernel: no ring entry, no spin"
    flat = [m for m in ins if m.startswith("flat_")]
    assert not flat, "%d flat instructions in %s: a hand-off word is reached through a generic pointer again (%s)" % (len(flat), kernel, sorted(set(flat)))
