"""The second launch of a split step (k_sweep_blc4, run_sweep_split) without a GPU: its resources in the built code object, and the schedule of
its completion signals played through on the host.

(i)  Both instances of k_sweep_blc4 keep four workgroups to a compute unit: at most 128 vector registers, no scratch memory, and static LDS
     that fits four times into a compute unit's 160 KB -- read from the library build_lib() links, so that an edit which tips the kernel over
     fails here.
(ii) A second launch carries a completion signal only where a wait reads it (sweep_blc_awaited, csrc/pf_pipe.h).  A stand-alone program -- its
     own main, compiled here for the host alone with the address and undefined-behaviour sanitizers, run as a process of its own -- plays
     run_sweep_split's order of launches, records and waits on a model of the sixteen events, for calls of 1 to 200 steps, every batch size,
     and behind an earlier call that left every entry recorded: each wait must meet the record of the very step it means, made in this
     call.  The test skips if the header cannot be compiled for the host alone."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLC4 = ("_Z12k_sweep_blc4ILb1EEvPK10SweepChunkx", "_Z12k_sweep_blc4ILb0EEvPK10SweepChunkx")       # k_sweep_blc4<true>, k_sweep_blc4<false>


@pytest.mark.parametrize("kernel", BLC4)
def test_second_launch_keeps_four_workgroups_per_cu(kernel):
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_meta
    from smcsmc_amd import build
    meta = kernel_meta.kernels(build.build_lib())
    assert kernel in meta, "the kernel was not found in the code object: " + ", ".join(sorted(k for k in meta if "blc4" in k))
    m = meta[kernel]
    assert m["vgpr"] + m["agpr"] <= 128, (kernel, m)
    assert m["scratch"] == 0, (kernel, m)
    assert 4 * m["lds"] <= 160 * 1024, (kernel, m)


PROGRAM = r"""
#include <cstdio>
#include <vector>
#include <hip/hip_runtime.h>
#include "pf_device.h"
using namespace pf;
#include "pf_pipe.h"

// what an entry of the event ring remembers: the call and the step of its last record (-1: never recorded)
struct Rec { int call = -1; long long step = -1; };

static int play(int call, long long steps, int batch, bool signal_all, std::vector<Rec>& ev, long long& signals) {
    int bad = 0;
    auto wait = [&](long long step, const char* who) {
        const Rec& r = ev[(size_t)(step & (PF_RING - 1))];
        if (r.call != call || r.step != step) {
            if (bad < 5) std::printf("steps %lld batch %d: %s waits for step %lld and meets call %d step %lld\n", steps, batch, who, step, r.call, r.step);
            ++bad;
        }
    };
    for (long long t = 0; t < steps; ++t) {
        if (const long long u = sweep_ring_awaited(t); u >= 0) wait(u, "the ring");
        const bool batch_end = ((t + 1) % batch) == 0 || t == steps - 1;
        if (batch_end)
            for (long long u = t - (t % batch); u <= t; ++u)
                if (signal_all || sweep_blc_awaited(u, steps)) { ev[(size_t)(u & (PF_RING - 1))] = Rec{call, u}; ++signals; }
    }
    wait(steps - 1, "the end of the call");
    return bad;
}

int main() {
    int bad = 0;
    long long sparse = 0, all = 0;
    for (int batch = 1; batch <= 4; ++batch)
        for (long long steps = 1; steps <= 200; ++steps)
            for (int mode = 0; mode < 2; ++mode) {
                std::vector<Rec> ev(PF_RING);
                long long n0 = 0;
                // an earlier call that left a record in every entry, then the call under test
                bad += play(0, 64 + steps % 16, batch, true, ev, n0);
                bad += play(1, steps, batch, mode == 1, ev, mode == 1 ? all : sparse);
            }
    // the ring waits look seven steps back, never further than the slots reach
    for (long long t = 0; t < 4096; ++t) {
        const long long u = sweep_ring_awaited(t);
        if (u >= 0 && (u != t - 7 || (t & 7) != 0)) { std::printf("ring wait of step %lld names step %lld\n", t, u); ++bad; }
        if (u < 0 && t >= 8 && (t & 7) == 0) { std::printf("no ring wait at step %lld\n", t); ++bad; }
    }
    std::printf("signals: %lld where read, %lld on every launch\n", sparse, all);
    if (!(sparse * 5 < all)) { std::printf("the sparse schedule signals more than one launch in five\n"); ++bad; }
    return bad ? 1 : 0;
}
"""


def test_signal_schedule_played_through(tmp_path):
    from smcsmc_amd import build
    src, exe = tmp_path / "schedule.hip", tmp_path / "schedule"
    src.write_text(PROGRAM)
    cmd = [build._hipcc(), "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I", build.CSRC, "-I", os.path.join(ROOT, "include"), "-x", "hip", str(src), "-o", str(exe), "-fsanitize=address,undefined"]
    cc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if cc.returncode != 0:
        pytest.skip("pf_pipe.h does not compile for the host alone here: " + cc.stderr[-400:])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "signals:" in r.stdout
