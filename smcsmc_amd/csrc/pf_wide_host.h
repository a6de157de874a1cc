// smcsmc_amd/csrc/pf_wide_host.h -- host entry points of the wide one-population kernels (pf_wide.hip): nsam up to
// PF_NMAX_WIDE, one wavefront per workgroup, 64-bit descendant masks, event records with the cut branch's samples in a word
// of their own (KArgs::RS = n + 5).  The kernels of the other steps (k_decide, k_resample, k_count<PF_NMAX_WIDE, 1>, k_ledger)
// are those of pf_hip.hip: they read the particle state from memory and take their particle ranges from their own launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "pf_types.h"

// dynamic LDS of the wide kernels: 3 (n - 1) doubles and 2 (n - 1) child ids per lane, 64 lanes, plus the epoch tables
size_t pf_wide_smem_bytes(int n, int E);
// raises the kernels' dynamic-LDS limit to `smem`; nonzero if that does not fit a workgroup
int pf_wide_prepare(size_t smem);
void pf_wide_launch_init(const KArgs& A, double initial_position, size_t smem, hipStream_t st);
void pf_wide_launch_extend(const KArgs& A, long long s, size_t smem, hipStream_t st);
void pf_wide_launch_calibrate(const KArgs& A, unsigned long long seed, long long rep0, long long nrep, int* out_epoch, double* out_dist,
                              size_t smem, hipStream_t st);
void pf_wide_launch_simulate(const KArgs& A, unsigned long long seed, int nchunks, long long max_sites, double* pos_out,
                             unsigned long long* mask_out, long long* n_out, size_t smem, hipStream_t st);
