/* blz_devalg.h -- launchers of the device block algebra kernels (blz_devalg.hip): C_k = X_k^T * Y for one or two X_k in one
 * pass, and Z_o = sum_t X_t * A_o,t mod p for one or two outputs in one pass, on a caller's blocks in device memory -- rows x n
 * u64 words, row stride ld, any row numbering (both operations are invariant under a permutation of the rows, so nothing is
 * imported into a slab).  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVALG_H
#define BLZ_DEVALG_H

#include "blz_kernels.h"

#define DEVALG_MAX_TERMS 4	/* = BLZ_MAX_TERMS of blz.h */

/* partial rows (nx * n * n words each) the scratch of launch_dev_dot must hold for width n, at either nx: the scratch of the
 * pair is exactly twice that of the single product */
int dev_dot_max_blocks(const KernelCfg &c, int n);

/* Blocks with the same pointer AND the same stride are one block, staged and read once; the same pointer with another stride
 * is a different block.  first[k] = the least j <= k such that block j is block k. */
void dev_same_blocks(int nb, const void *const *b, const long long *ld, int *first);

/* out[e] = sum_b partial[b][e] mod p, e < words; nblocks == 0: zeros.  The second launch of every inner product. */
hipError_t launch_dev_dot_finalize(const u64 *partial, int nblocks, int words, u64 p, u64 *out, hipStream_t s);

/* out[k * n * n + i * n + j] = sum_r x[k][r * ldx[k] + i] * y[r * ldy + j] mod p for k < nx, nx = 1 (blz_dot_device) or 2
 * (blz_dot_pair_device).  Every workgroup writes one row of nx * n * n residues ([panel][entry]) to `partial` (room for
 * dev_dot_max_blocks() rows), a second launch adds the rows mod p into `out`; rows == 0: out = 0.  The Barrett class of
 * 2^32 <= p has no paired kernel at n > 32 (two sets of 16 128-bit accumulators do not fit a lane's 256 registers): there
 * nx = 2 runs the single form twice inside the one call.  n is the caller's width (1 .. 64), not c.n; of c only the modulus,
 * its reducer class and the CU count are read. */
hipError_t launch_dev_dot(const KernelCfg &c, int n, long long rows, int nx, const u64 *const *x, const long long *ldx,
			  const u64 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s);

/* z0[r * ldz0 + j] = sum_t sum_i x[t][r * ldx[t] + i] * a0[t][i * n + j] mod p, 1 <= nterms <= DEVALG_MAX_TERMS; nz = 2
 * (blz_combine_pair_device): z1 the same with a1, each sum over the terms whose panel is not NULL, every term in at least one
 * output and every output with at least one term.  ONE launch at every width and panel count: a lane group reads its row of
 * every term before it writes an output row, so each output may BE one of the x[t] (same pointer, same stride).  At nz = 2 the
 * coefficient panels sit in LDS as far as 160 KB go; the terms whose panels do not fit read theirs from global memory. */
hipError_t launch_dev_combine(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			      int nz, const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
			      hipStream_t s);

#endif
