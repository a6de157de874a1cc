// smcsmc_amd/csrc/pf_probe.hip -- measurement probe, not part of the filter: what does it cost to hand a row over from the
// extend workgroups of row s to those of row s + 1?
//
// The row pipeline pays a kernel boundary per row (pf_hip.hip, k_sweep): the 157 wavefronts of C3's 40 extend workgroups leave
// five partial sums each, the launch ends, the next launch's workgroups read the 785 numbers and redo the row's decision.  The
// alternative is a grid that stays resident: every wavefront publishes its partials with release stores, bumps an arrival
// counter, polls it, then reads the others' partials with coherent loads.  DESIGN.md priced that hand-off from the guide's
// table in round 3; pf_probe_handoff measures both forms on the device, with the same reduction of the same 785 numbers and a
// chosen amount of work per row in between, so that the figure that decides the question is a measurement.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pf_tree_reg.h"

namespace {

constexpr int NPART = 5;

__device__ __forceinline__ void spin_100mhz(long long ticks) {
    if (ticks <= 0) return;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(1);
}

// the reduction every workgroup redoes from all wavefronts' partials (decide_row's shape: three levels of a radix-64 tree)
__device__ __forceinline__ double reduce_partials(const double* part, int nw, bool coherent) {
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int k = lane; k < nw * NPART; k += 64) {
        const double v = coherent ? __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : part[k];
        acc += v;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
    return acc;
}

// one launch per row: the partials of the previous row are in memory (kernel boundary), this row's are written at the end
__global__ __launch_bounds__(256) void k_handoff_launch(const double* prev, double* next, int nw, long long spin, double* out, int row) {
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double acc = reduce_partials(prev, nw, false);
    spin_100mhz(spin);
    if (gw < nw && lane < NPART) next[gw * NPART + lane] = acc * 1e-3 + (double)(gw + lane + row);
    if (gw < nw && lane == 0) out[gw] = acc;
}

// resident grid: rows in a loop, hand-off through an arrival counter per row
__global__ __launch_bounds__(256) void k_handoff_resident(double* part /* [2][nw * NPART] */, unsigned* arrive /* [rows] */, int nw, int rows,
                                                          long long spin, double* out, int* err) {
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int r = 0; r < rows; ++r) {
        double* mine = part + (size_t)(r & 1) * nw * NPART;
        spin_100mhz(spin);
        if (gw < nw && lane < NPART) __hip_atomic_store(&mine[gw * NPART + lane], acc * 1e-3 + (double)(gw + lane + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gw < nw) {
            if (lane == 0) {
                __hip_atomic_fetch_add(&arrive[r], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);      // after this wavefront's partials
                int guard = 0;
                while (__hip_atomic_load(&arrive[r], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)nw) {
                    if (++guard > 4000000) { *err = 1; break; }       // a grid that is not resident as a whole must not hang the box
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;       // somebody gave up waiting: everybody leaves
        acc = reduce_partials(mine, nw, true);
    }
    if (gw < nw && lane == 0) out[gw] = acc;
}

// the same with the hand-off done per workgroup: one arrival and one poller per workgroup (the other wavefronts wait at the
// workgroup barrier), the partials fetched once per workgroup into LDS
__global__ __launch_bounds__(256) void k_handoff_resident_wg(double* part, unsigned* arrive, int nw, int rows, long long spin, double* out, int* err) {
    __shared__ double s_part[4096];
    __shared__ int s_bad;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nwg = (int)gridDim.x, np = nw * NPART;
    double acc = 0.0;
    if (threadIdx.x == 0) s_bad = 0;
    for (int r = 0; r < rows; ++r) {
        double* mine = part + (size_t)(r & 1) * np;
        spin_100mhz(spin);
        if (gw < nw && lane < NPART) __hip_atomic_store(&mine[gw * NPART + lane], acc * 1e-3 + (double)(gw + lane + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add(&arrive[r], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            int guard = 0;
            while (__hip_atomic_load(&arrive[r], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)nwg) {
                if (++guard > 4000000) { *err = 1; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) s_bad = 1;
        }
        __syncthreads();
        if (s_bad) break;
        for (int k = threadIdx.x; k < np && k < 4096; k += 256) s_part[k] = __hip_atomic_load(&mine[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        double a2 = 0.0;
        for (int k = lane; k < np && k < 4096; k += 64) a2 += s_part[k];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) a2 += __shfl_xor(a2, m, 64);
        acc = a2;
        __syncthreads();
    }
    if (gw < nw && lane == 0) out[gw] = acc;
}

// One case per lane: the selection and the edit of a genealogy update at four haplotypes, by the general form (form 0) and by
// the by-case form of the row kernel (form 1).  oi[form][case][10] = rp, sb, descendants of the cut branch, the six children (rank
// by rank, child 0 then 1), changed; od[form][case][4] = the three heights and the height of the removed node.
__global__ __launch_bounds__(256) void k_tree_edit4(int ncases, const double* S, const int32_t* Cin, const double* h, const int32_t* lin,
                                                    const int32_t* rp, const int32_t* sb, const double* tc, const double* u_attach,
                                                    int32_t* oi, double* od) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncases) return;
#pragma unroll
    for (int form = 0; form < 2; ++form) {
        pf::RTree<4> t;
#pragma unroll
        for (int r = 0; r < 3; ++r) { t.S[r] = S[(size_t)3 * i + r]; t.C0[r] = Cin[(size_t)6 * i + 2 * r]; t.C1[r] = Cin[(size_t)6 * i + 2 * r + 1]; }
        int s_rp = 0, s_sb = 0;
        unsigned desc = 0;
        double Sp = 0.0;
        bool changed = false;
        if (form == 0) {
            pf::RCtx cx = {};
            cx.n = 4; cx.want_desc = true;
            unsigned tmask[7];
            pf::r_update_select<4>(cx, t, 4, h[i], lin[i], false, true, &s_rp, &s_sb, tmask);
            desc = cx.last_desc;
            pf::r_update_edit<4>(cx, t, 4, rp[i], sb[i], tc[i], u_attach[i], tmask, &Sp, &changed);
        } else {
            pf::r4_select(t, h[i], lin[i], &s_rp, &s_sb, &desc);
            pf::r4_edit(t, rp[i], sb[i], tc[i], u_attach[i], &Sp, &changed);
        }
        int32_t* o = oi + ((size_t)form * ncases + i) * 10;
        o[0] = s_rp; o[1] = s_sb; o[2] = (int32_t)desc;
#pragma unroll
        for (int r = 0; r < 3; ++r) { o[3 + 2 * r] = t.C0[r]; o[4 + 2 * r] = t.C1[r]; }
        o[9] = changed ? 1 : 0;
        double* d = od + ((size_t)form * ncases + i) * 4;
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = t.S[r];
        d[3] = Sp;
    }
}

// One wavefront per 64 values: every wavefront primitive of pf_device.h in its *_lds form (form 0) and in the form without LDS (form 1).
// od[form][0..3][i] = wave_tree_sum, wave_hs_scan, wave_max_scan_d, the value of the lane before (shift by one, lane 0 its own);
// oi[form][0..3][i] = wave_max_scan_i, the minimum and the maximum of wave_minmax, the value of the lane before.
__global__ __launch_bounds__(256) void k_wave_prims(int nwaves, const double* xd, const int32_t* xi, double* od, int32_t* oi) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)nwaves * 64;
    const int lane = threadIdx.x & 63;
    if (i >= n) return;                   // (whole wavefronts: n is a multiple of 64)
    const double v = xd[i];
    const int k = xi[i];
    od[(0 * 4 + 0) * n + i] = pf::wave_tree_sum_lds(v);
    od[(0 * 4 + 1) * n + i] = pf::wave_hs_scan_lds(v, lane);
    od[(0 * 4 + 2) * n + i] = pf::wave_max_scan_d_lds(v, lane);
    od[(0 * 4 + 3) * n + i] = __shfl_up(v, 1, 64);
    od[(1 * 4 + 0) * n + i] = pf::wave_tree_sum(v);
    od[(1 * 4 + 1) * n + i] = pf::wave_hs_scan(v, lane);
    od[(1 * 4 + 2) * n + i] = pf::wave_max_scan_d(v, lane);
    od[(1 * 4 + 3) * n + i] = pf::wave_prev_lane(v, v);
    int mn = k, mx = k;
    pf::wave_minmax_lds(mn, mx);
    oi[(0 * 4 + 0) * n + i] = pf::wave_max_scan_i_lds(k, lane);
    oi[(0 * 4 + 1) * n + i] = mn;
    oi[(0 * 4 + 2) * n + i] = mx;
    oi[(0 * 4 + 3) * n + i] = __shfl_up(k, 1, 64);
    mn = k; mx = k;
    pf::wave_minmax(mn, mx);
    oi[(1 * 4 + 0) * n + i] = pf::wave_max_scan_i(k, lane);
    oi[(1 * 4 + 1) * n + i] = mn;
    oi[(1 * 4 + 2) * n + i] = mx;
    oi[(1 * 4 + 3) * n + i] = pf::wave_prev_lane(k, k);
}

}  // namespace

// mode 0: `rows` launches of k_handoff_launch back to back on one stream; mode 1: one launch of the resident grid, every wavefront
// arriving and polling for itself; mode 2: the resident grid with one arrival and one poller per workgroup.
// nw wavefronts in workgroups of four; spin_ticks of 10 ns of stand-in work per wavefront and row.  Returns microseconds per row
// (HIP events around the whole sequence) in *us_per_row and a checksum (the two modes compute the same numbers).
extern "C" int pf_probe_handoff(int32_t mode, int32_t rows, int32_t nw, int64_t spin_ticks, double* us_per_row, double* checksum, int32_t device) {
    if (rows < 1 || nw < 1 || nw > 4096 || (mode == 2 && nw * NPART > 4096)) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    const int nwg = (nw + 3) / 4;
    double *part = nullptr, *out = nullptr;
    unsigned* arrive = nullptr;
    int* err = nullptr;
    hipStream_t st;
    hipEvent_t e0, e1;
    if (hipMalloc(&part, (size_t)2 * nw * NPART * 8) != hipSuccess || hipMalloc(&out, (size_t)nw * 8) != hipSuccess ||
        hipMalloc(&arrive, (size_t)rows * 4) != hipSuccess || hipMalloc(&err, 4) != hipSuccess) return -1;
    hipMemset(part, 0, (size_t)2 * nw * NPART * 8); hipMemset(arrive, 0, (size_t)rows * 4); hipMemset(err, 0, 4); hipMemset(out, 0, (size_t)nw * 8);
    hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipDeviceSynchronize();
    // warm-up launch of either kernel (code object load), outside the timed region
    if (mode == 0) hipLaunchKernelGGL(k_handoff_launch, dim3(nwg), dim3(256), 0, st, part, part + (size_t)nw * NPART, nw, 0LL, out, -1);
    hipStreamSynchronize(st);
    hipMemset(part, 0, (size_t)2 * nw * NPART * 8);
    hipEventRecord(e0, st);
    if (mode == 0) {
        for (int r = 0; r < rows; ++r) {
            double* prev = part + (size_t)((r + 1) & 1) * nw * NPART;
            double* next = part + (size_t)(r & 1) * nw * NPART;
            hipLaunchKernelGGL(k_handoff_launch, dim3(nwg), dim3(256), 0, st, prev, next, nw, (long long)spin_ticks, out, r);
        }
    } else if (mode == 1) {
        hipLaunchKernelGGL(k_handoff_resident, dim3(nwg), dim3(256), 0, st, part, arrive, nw, rows, (long long)spin_ticks, out, err);
    } else {
        hipLaunchKernelGGL(k_handoff_resident_wg, dim3(nwg), dim3(256), 0, st, part, arrive, nw, rows, (long long)spin_ticks, out, err);
    }
    hipEventRecord(e1, st);
    if (mode == 0)          // (untimed) the reduction of the last row's partials, which the resident grid has already done
        hipLaunchKernelGGL(k_handoff_launch, dim3(nwg), dim3(256), 0, st, part + (size_t)((rows + 1) & 1) * nw * NPART, part + (size_t)(rows & 1) * nw * NPART, nw, 0LL, out, rows);
    const hipError_t rc = hipStreamSynchronize(st);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<double> h(nw);
    int herr = 0;
    hipMemcpy(h.data(), out, (size_t)nw * 8, hipMemcpyDeviceToHost);
    hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost);
    double cs = 0.0;
    for (double v : h) cs += v;
    if (us_per_row) *us_per_row = 1e3 * (double)ms / rows;
    if (checksum) *checksum = cs;
    hipFree(part); hipFree(out); hipFree(arrive); hipFree(err);
    hipEventDestroy(e0); hipEventDestroy(e1); hipStreamDestroy(st);
    return (rc == hipSuccess && herr == 0) ? 0 : -2;
}

// The two forms of the integer part of a genealogy update at four haplotypes, side by side on cases from the host (k_tree_edit4
// above; not part of the filter, no timing).  Per case: the tree (S[3] ascending, C[6]), a point (h, lin) for the selection, and a
// cut branch (rp, sb), a coalescence time tc and the uniform u_attach for the edit.  out_i[2][ncases][10], out_d[2][ncases][4].
extern "C" int pf_probe_tree_edit(int32_t ncases, const double* S, const int32_t* C, const double* h, const int32_t* lin, const int32_t* rp,
                                   const int32_t* sb, const double* tc, const double* u_attach, int32_t* out_i, double* out_d, int32_t device) {
    if (ncases < 1 || ncases > (1 << 24)) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    const size_t nc = (size_t)ncases;
    const void* src[8] = {S, C, h, lin, rp, sb, tc, u_attach};
    const size_t bytes[8] = {nc * 3 * 8, nc * 6 * 4, nc * 8, nc * 4, nc * 4, nc * 4, nc * 8, nc * 8};
    void* d[8] = {};
    int32_t* d_oi = nullptr;
    double* d_od = nullptr;
    bool ok = true;
    for (int k = 0; k < 8 && ok; ++k)
        ok = hipMalloc(&d[k], bytes[k]) == hipSuccess && hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMalloc(&d_oi, nc * 2 * 10 * 4) == hipSuccess && hipMalloc(&d_od, nc * 2 * 4 * 8) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_tree_edit4, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, 0, ncases, (const double*)d[0], (const int32_t*)d[1],
                           (const double*)d[2], (const int32_t*)d[3], (const int32_t*)d[4], (const int32_t*)d[5], (const double*)d[6],
                           (const double*)d[7], d_oi, d_od);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out_i, d_oi, nc * 2 * 10 * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(out_d, d_od, nc * 2 * 4 * 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    for (int k = 0; k < 8; ++k) if (d[k]) hipFree(d[k]);
    if (d_oi) hipFree(d_oi);
    if (d_od) hipFree(d_od);
    return ok ? 0 : -2;
}

// The wavefront primitives of pf_device.h, both forms side by side (k_wave_prims above; not part of the filter, no timing): nwaves
// wavefronts of 64 doubles xd and 64 integers xi from the host.  out_d[2][4][nwaves * 64], out_i[2][4][nwaves * 64].
extern "C" int pf_probe_wave_prims(int32_t nwaves, const double* xd, const int32_t* xi, double* out_d, int32_t* out_i, int32_t device) {
    if (nwaves < 1 || nwaves > (1 << 18)) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    const size_t n = (size_t)nwaves * 64;
    double *d_xd = nullptr, *d_od = nullptr;
    int32_t *d_xi = nullptr, *d_oi = nullptr;
    bool ok = hipMalloc(&d_xd, n * 8) == hipSuccess && hipMalloc(&d_xi, n * 4) == hipSuccess && hipMalloc(&d_od, n * 8 * 8) == hipSuccess &&
              hipMalloc(&d_oi, n * 8 * 4) == hipSuccess && hipMemcpy(d_xd, xd, n * 8, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_xi, xi, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_wave_prims, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, nwaves, (const double*)d_xd, (const int32_t*)d_xi, d_od, d_oi);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out_d, d_od, n * 8 * 8, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(out_i, d_oi, n * 8 * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (d_xd) hipFree(d_xd);
    if (d_xi) hipFree(d_xi);
    if (d_od) hipFree(d_od);
    if (d_oi) hipFree(d_oi);
    return ok ? 0 : -2;
}
