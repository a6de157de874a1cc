// smcsmc_amd/csrc/pf_wide.hip -- the one-population LDS-tree kernels for up to PF_NMAX_WIDE (64) haplotypes.
//
// The bodies are those of k_init / k_extend / k_calibrate / k_simulate (pf_lds_body.h), compiled here with one wavefront per
// workgroup and 64-bit masks.  A lane's tree columns are 3 (n - 1) doubles and 2 (n - 1) child ids at a stride of the workgroup
// size: at n = 64 that is 104 KB of LDS for 64 lanes (one workgroup per compute unit), where 256 lanes would need 410 KB.
// The per-wavefront partials of k_extend (chunk = p >> 6) do not depend on the workgroup size, so k_decide / k_resample /
// k_count of pf_hip.hip consume them as they are.
#define PF_BS 64
#define PF_WIDE 1
#define PF_MASK_T unsigned long long
#include <hip/hip_runtime.h>

#include "pf_device.h"
#include "pf_types.h"
#include "pf_lane.h"
#include "pf_row_parts.h"
#include "pf_lds_body.h"
#include "pf_wide_host.h"

__global__ __launch_bounds__(PF_BS) void k_init_wide(KArgs A, double initial_position) {
    extern __shared__ double smem[];
    init_lds_body(A, initial_position, smem);
}

__global__ __launch_bounds__(PF_BS) void k_extend_wide(KArgs A, long long s) {
    extern __shared__ double smem[];
    extend_lds_body(A, s, smem);
}

__global__ __launch_bounds__(PF_BS) void k_calibrate_wide(KArgs A, unsigned long long seed, long long rep0, long long nrep,
                                                          int* out_epoch, double* out_dist) {
    extern __shared__ double smem[];
    calibrate_lds_body<0>(A, seed, rep0, nrep, out_epoch, out_dist, smem);
}

__global__ __launch_bounds__(PF_BS) void k_simulate_wide(KArgs A, unsigned long long seed, int nchunks, long long max_sites,
                                                         double* pos_out, unsigned long long* mask_out, long long* n_out) {
    extern __shared__ double smem[];
    simulate_lds_body(A, seed, nchunks, max_sites, pos_out, mask_out, n_out, smem);
}

size_t pf_wide_smem_bytes(int n, int E) { return smem_bytes(n, E); }

int pf_wide_prepare(size_t smem) {
    if (smem > 160 * 1024) return -1;
    if (smem > 64 * 1024) {
        const void* ks[4] = {(const void*)k_init_wide, (const void*)k_extend_wide, (const void*)k_calibrate_wide, (const void*)k_simulate_wide};
        for (const void* k : ks)
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return -1;
    }
    return 0;
}

static unsigned wide_grid(long long lanes) { return (unsigned)((lanes + PF_BS - 1) / PF_BS); }

void pf_wide_launch_init(const KArgs& A, double initial_position, size_t smem, hipStream_t st) {
    hipLaunchKernelGGL(k_init_wide, dim3(wide_grid(A.Np)), dim3(PF_BS), smem, st, A, initial_position);
}

void pf_wide_launch_extend(const KArgs& A, long long s, size_t smem, hipStream_t st) {
    hipLaunchKernelGGL(k_extend_wide, dim3(wide_grid(A.Np)), dim3(PF_BS), smem, st, A, s);
}

void pf_wide_launch_calibrate(const KArgs& A, unsigned long long seed, long long rep0, long long nrep, int* out_epoch, double* out_dist,
                              size_t smem, hipStream_t st) {
    hipLaunchKernelGGL(k_calibrate_wide, dim3(wide_grid(nrep)), dim3(PF_BS), smem, st, A, seed, rep0, nrep, out_epoch, out_dist);
}

void pf_wide_launch_simulate(const KArgs& A, unsigned long long seed, int nchunks, long long max_sites, double* pos_out,
                             unsigned long long* mask_out, long long* n_out, size_t smem, hipStream_t st) {
    hipLaunchKernelGGL(k_simulate_wide, dim3(wide_grid(nchunks)), dim3(PF_BS), smem, st, A, seed, nchunks, max_sites, pos_out, mask_out, n_out);
}
