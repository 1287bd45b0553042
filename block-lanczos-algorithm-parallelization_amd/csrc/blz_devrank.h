/* blz_devrank.h -- launchers of the rank-local device-block kernels (blz_devrank.hip): a rank's own rows of a whole block,
 * taken out of it and put back, and the last step of an inner product summed over ranks.  C++ side only; not part of the
 * C ABI. */
#ifndef BLZ_DEVRANK_H
#define BLZ_DEVRANK_H

#include "blz_kernels.h"

/* local[q][0..n) <- whole[id(q)][0..n) for q in [0, rows), id(q) = inv ? inv[first + q] : first + q: the rank's rows in slab
 * order out of a block in the file's numbering.  Both sides are u64 words, row strides ldl, ldw >= n; the words past n of a
 * row are neither read nor written.  inv: the whole side's numbering on the device (nullptr: the identity). */
hipError_t launch_rows_take(const KernelCfg &c, u64 *local, long long ldl, const u64 *whole, long long ldw, const int *inv,
			    long long first, long long rows, int n, hipStream_t s);
/* whole[id(q)][0..n) <- local[q][0..n): the reverse; no other row of `whole` is written */
hipError_t launch_rows_put(const KernelCfg &c, u64 *whole, long long ldw, const u64 *local, long long ldl, const int *inv,
			   long long first, long long rows, int n, hipStream_t s);
/* out[i] <- sums[i] mod p for i in [0, words): sums of at most nranks residues, nranks * p <= 2^64, so no sum has wrapped */
hipError_t launch_residue_sums(const KernelCfg &c, u64 *out, const u64 *sums, int words, hipStream_t s);

#endif
