/* blz_devalg.h -- launchers of the device block algebra kernels (blz_devalg.hip): C = X^T * Y and Z = sum_t X_t * A_t mod p on
 * a caller's blocks in device memory -- rows x n u64 words, row stride ld, any row numbering (both operations are invariant
 * under a permutation of the rows, so nothing is imported into a slab).  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVALG_H
#define BLZ_DEVALG_H

#include "blz_kernels.h"

#define DEVALG_MAX_TERMS 4	/* = BLZ_MAX_TERMS of blz.h */

/* partial rows (n * n words each) the scratch of launch_dev_dot must hold for width n */
int dev_dot_max_blocks(const KernelCfg &c, int n);

/* out[i * n + j] = sum_r x[r * ldx + i] * y[r * ldy + j] mod p.  Every workgroup writes one row of n * n residues to
 * `partial` (room for dev_dot_max_blocks() rows), a second launch adds the rows mod p into `out`; rows == 0: out = 0.
 * n is the caller's width (1 .. 64), not c.n; of c only the modulus, its reducer class and the CU count are read. */
hipError_t launch_dev_dot(const KernelCfg &c, int n, long long rows, const u64 *x, long long ldx, const u64 *y, long long ldy,
			  u64 *partial, u64 *out, hipStream_t s);

/* z[r * ldz + j] = sum_t sum_i x[t][r * ldx[t] + i] * a[t][i * n + j] mod p, 1 <= nterms <= DEVALG_MAX_TERMS.  A lane group
 * reads its row of every term before it writes the row of z: z may BE one or more of the x[t] (same pointer, same stride). */
hipError_t launch_dev_combine(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			      const u64 *const *a, u64 *z, long long ldz, hipStream_t s);

#endif
