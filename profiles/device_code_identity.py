"""Device code of two builds of libsmcsmc_pf.so, kernel by kernel (the method of profiles/round10/device_code_identity.md):

    python profiles/device_code_identity.py PARENT.so THIS.so > profiles/roundNN/device_code_identity.md

Both libraries have to be built at the same path (hipcc derives a symbol from the path of each source file).  For every clang offload
bundle of the .hip_fatbin section (pf_hip, pf_mp, pf_wide, pf_probe, in link order) the gfx950 code object is taken out; for every kernel
of the parent the `llvm-objdump -d` text, its trailing `// address: encoding` comments and the padding behind its last `s_endpgm` stripped, and the figures of the AMDGPU metadata
note (tests/tools/kernel_meta.py) are compared with this tree's.  Kernels only this tree has are listed with their figures.  Needs no GPU."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import kernel_meta  # noqa: E402

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
UNITS = ("pf_hip", "pf_mp", "pf_wide", "pf_probe")


def objdump():
    for cand in ("/opt/rocm/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objdump"):
        if os.path.exists(cand):
            return cand
    return "llvm-objdump"


def bundles(lib):
    """per bundle: (gfx950 ELF bytes, kernel_meta figures)"""
    b = open(lib, "rb").read()
    out = []
    i = b.find(MAGIC)
    while i >= 0:
        n = struct.unpack_from("<Q", b, i + 24)[0]
        off = i + 32
        elf = None
        for _ in range(n):
            o, sz, ts = struct.unpack_from("<QQQ", b, off)
            off += 24
            if "gfx950" in b[off:off + ts].decode():
                elf = b[i + o:i + o + sz]
            off += ts
        with tempfile.NamedTemporaryFile(suffix=".bundle") as t:      # kernel_meta reads the first bundle of the file it is given
            t.write(b[i:]); t.flush()
            meta = kernel_meta.kernels(t.name)
        out.append((elf, meta))
        i = b.find(MAGIC, i + len(MAGIC))
    return out


def disassembly(elf):
    """symbol -> instruction text without addresses"""
    with tempfile.NamedTemporaryFile(suffix=".co") as t:
        t.write(elf); t.flush()
        text = subprocess.run([objdump(), "-d", t.name], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = m.group(1); out[cur] = []
        elif cur is not None and ln.strip():
            out[cur].append(re.sub(r"\s*//.*$", "", ln).strip())
    # what follows the last s_endpgm is padding up to the next kernel's alignment: it depends on where the kernel lies, not on its code
    # (s_nop 0, a "..." of the disassembler, or the kernel descriptor of the next symbol decoded as if it were code)
    for k, v in out.items():
        if "s_endpgm" in v:
            del v[len(v) - v[::-1].index("s_endpgm"):]
    return out


def same_kernel_renamed(name, theirs):
    """A kernel of the parent that became a template, or gained a template argument, with the value it had built in (the population width
    PF_PMAX = 4 of the structured walk, round 23) keeps its code under another mangled name: k<..., 4> for k<...>, k<4> for k."""
    for t in theirs:
        for was in (t.replace("ELi4EEv", "EEv"), t.replace("ILi4EEv", "").replace("S1_", "S0_")):
            if was == name and t != name:
                return t
    return None


def main(parent, this):
    pb, tb = bundles(parent), bundles(this)
    assert len(pb) == len(tb) == len(UNITS), (len(pb), len(tb))
    print("| bundle | kernels of the parent | with a differing instruction | with differing figures | kernels only this tree has |")
    print("|---|---|---|---|---|")
    changed, added, renamed = [], [], []
    for name, (pe, pm), (te, tm) in zip(UNITS, pb, tb):
        pd, td = disassembly(pe), disassembly(te)
        for k in [k for k in pm if k not in tm]:
            t = same_kernel_renamed(k, tm)
            if t:
                renamed.append((name, k, t))
                tm[k], td[k] = tm.pop(t), td.pop(t)
        diff_i = [k for k in pm if pd.get(k) != td.get(k)]
        diff_m = [k for k in pm if pm[k] != tm.get(k)]
        new = sorted(k for k in tm if k not in pm)
        print("| `%s` | %d | %d | %d | %d |" % (name, len(pm), len(diff_i), len(diff_m), len(new)))
        changed += [(name, k, pm[k], tm.get(k), len(pd.get(k, [])), len(td.get(k, []))) for k in sorted(set(diff_i) | set(diff_m))]
        added += [(name, k, tm[k], len(td.get(k, []))) for k in new]
    print()
    if changed:
        print("Kernels of the parent that changed:\n")
        for name, k, a, b, na, nb in changed:
            print("- `%s` `%s`: %s, %d lines -> %s, %d lines" % (name, k, a, na, b, nb))
    else:
        print("Every kernel of the parent has the parent's instruction text, line for line, and the parent's VGPR, AGPR, SGPR, LDS and scratch figures.")
    if renamed:
        print("\nKernels compared under the name they have now (same code, one more template argument in the mangled name):\n")
        for name, k, t in renamed:
            print("- `%s` `%s` is now `%s`" % (name, k, t))
    print("\nKernels only this tree has:\n")
    print("| bundle | kernel | VGPR | AGPR | SGPR | static LDS | scratch | instructions |")
    print("|---|---|---|---|---|---|---|---|")
    for name, k, m, nl in added:
        print("| `%s` | `%s` | %d | %d | %d | %d | %d | %d |" % (name, k, m["vgpr"], m["agpr"], m["sgpr"], m["lds"], m["scratch"], nl))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
