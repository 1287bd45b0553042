/* blz_devfuse.h -- launchers of the fused device block algebra kernels (blz_devfuse.hip): two inner products against one
 * block in one pass, and two recombinations of shared inputs in one pass, on a caller's blocks in device memory -- rows x n u64
 * words, row stride ld, the conventions of blz_devalg.h.  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVFUSE_H
#define BLZ_DEVFUSE_H

#include "blz_devalg.h"

/* partial rows (2 * n * n words each) the scratch of launch_dev_dot2 must hold for width n: dev_dot_max_blocks() of them, so
 * the scratch is exactly twice that of launch_dev_dot */
int dev_dot2_max_blocks(const KernelCfg &c, int n);

/* 1 where width n runs k_dev_dot2, 0 where launch_dev_dot2 issues launch_dev_dot twice: n > 32 in the Barrett class of
 * 2^32 <= p, where two sets of 16 128-bit accumulators do not fit a lane's 256 registers */
int dev_dot2_fused(const KernelCfg &c, int n);

/* out[i * n + j] = sum_r x0[r * ldx0 + i] * y[r * ldy + j] mod p and out[n * n + i * n + j] the same with x1.  Blocks that are
 * the same pointer with the same stride are staged and read once.  `partial` has room for dev_dot2_max_blocks() rows of
 * 2 * n * n words; a second launch adds the rows mod p into `out`; rows == 0: out = 0. */
hipError_t launch_dev_dot2(const KernelCfg &c, int n, long long rows, const u64 *x0, long long ldx0, const u64 *x1, long long ldx1,
			   const u64 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s);

/* z0[r * ldz0 + j] = sum_t sum_i x[t][r * ldx[t] + i] * a0[t][i * n + j] mod p over the terms with a0[t] != NULL, z1 the same
 * with a1; 1 <= nterms <= DEVALG_MAX_TERMS, every term in at least one output and every output with at least one term.  ONE
 * launch at every width and panel count: a lane group reads its row of every term before it writes either output row, so each
 * of z0 and z1 may BE one of the x[t] (same pointer, same stride).  The coefficient panels sit in LDS as far as 160 KB go; the
 * terms whose panels do not fit read theirs from global memory. */
hipError_t launch_dev_combine2(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			       const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
			       hipStream_t s);

#endif
