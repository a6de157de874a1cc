#!/usr/bin/env python3
"""The entry of k_sweep_blc4 in the ISA, parent and new, from the pf_hip objects the two libraries were linked from (no GPU needed):

    python profiles/count_chain_isa.py <parent checkout>/smcsmc_amd/csrc/build/pf_hip.o smcsmc_amd/csrc/build/pf_hip.o

For each instance and side: the scalar loads and waits in layout order from the entry of the kernel to its first vector memory instruction
(every workgroup of the launch runs through them: the entry is one straight line up to the branch on the workgroup's role), the totals of the
whole kernel, and the registers, LDS and scratch memory from the kernel descriptor's metadata.  Prints markdown."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "tools"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from smcsmc_amd import build  # noqa: E402

KERNELS = {"k_sweep_blc4<true>": "_Z12k_sweep_blc4ILb1EEvPK10SweepChunkx", "k_sweep_blc4<false>": "_Z12k_sweep_blc4ILb0EEvPK10SweepChunkx"}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    hipcc = os.path.realpath(build._hipcc())
    root = os.path.dirname(os.path.dirname(hipcc))
    for d in (os.path.dirname(hipcc), os.path.join(root, "lib", "llvm", "bin"), os.path.join(root, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise SystemExit(name + " not found beside hipcc")


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".hipfb"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, tag + ".copy.o")])
    subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co])
    return co


def listing(co, sym):
    text = subprocess.check_output([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + sym, co], text=True)
    return [re.sub(r"\s*//.*$", "", ln).strip() for ln in text.splitlines() if re.match(r"^\s+[a-z]", ln)]


def is_vmem(ins):
    return ins.startswith(("global_", "flat_", "buffer_", "scratch_"))


def describe(ins):
    head = []
    for i in ins:
        if is_vmem(i):
            break
        head.append(i)
    return dict(head=head, n=len(ins),
                head_sloads=sum(1 for i in head if i.startswith("s_load")), head_waits=sum(1 for i in head if i.startswith("s_waitcnt") and "lgkmcnt(0)" in i),
                sloads=sum(1 for i in ins if i.startswith("s_load")), waits=sum(1 for i in ins if i.startswith("s_waitcnt") and "lgkmcnt(0)" in i),
                vm_loads=sum(1 for i in ins if is_vmem(i) and "_load" in i), barriers=sum(1 for i in ins if i.startswith("s_barrier")))


def main():
    import kernel_meta
    sides = {"parent": sys.argv[1], "new": sys.argv[2]}
    with tempfile.TemporaryDirectory() as tmp:
        cos = {k: code_object(v, tmp, k) for k, v in sides.items()}
        for name, sym in KERNELS.items():
            d = {k: describe(listing(co, sym)) for k, co in cos.items()}
            m = {k: kernel_meta.kernels(obj)[sym] for k, obj in sides.items()}
            print("## `%s`\n" % name)
            print("| | parent | new |\n|---|---|---|")
            rows = [("instructions", "n"), ("scalar loads before the first vector memory instruction", "head_sloads"),
                    ("`s_waitcnt lgkmcnt(0)` before the first vector memory instruction", "head_waits"), ("scalar loads, whole kernel", "sloads"),
                    ("`s_waitcnt lgkmcnt(0)`, whole kernel", "waits"), ("vector loads, whole kernel", "vm_loads"), ("`s_barrier`", "barriers")]
            for what, key in rows:
                print("| %s | %d | %d |" % (what, d["parent"][key], d["new"][key]))
            for what, key in (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs", "sgpr"), ("static LDS, bytes", "lds"), ("scratch, bytes", "scratch")):
                print("| %s | %d | %d |" % (what, m["parent"][key], m["new"][key]))
            for k in ("parent", "new"):
                print("\nThe entry, %s (scalar loads and waits in layout order up to the first vector memory instruction):\n\n```" % k)
                for i in d[k]["head"]:
                    if i.startswith(("s_load", "s_waitcnt", "s_cbranch", "s_branch", "s_endpgm")):
                        print(i)
                print("```")
            print()


if __name__ == "__main__":
    main()
