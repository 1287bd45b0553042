/* blz_devmat.h -- launchers of the device matrix build (blz_devmat.hip): CSR(M) and CSR(M^T) made on the GPU from a caller's
 * triplets (blz_set_matrix_device / blz_set_matrix_upload).  Three passes, as the host build's
 * (csrc/host/blz_host.c, csr_from_coo_window): check + histogram, exclusive scan, scatter through per-row cursors -- then, for a
 * slab that can be packed, the palette and the rewrite of col_idx.  Passes are ordered by kernel boundaries alone.
 * C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVMAT_H
#define BLZ_DEVMAT_H

#include "blz_kernels.h"

/* the scan: a workgroup takes DEVMAT_SCAN_TILE counters; the one workgroup that scans the tile sums takes them
 * DEVMAT_SCAN_CHUNK at a time (tests/device_matrix_ref.py restates both) */
#define DEVMAT_SCAN_TILE 1024
#define DEVMAT_SCAN_CHUNK 256

/* what the check pass counts, in this order (device words of unsigned long long, zeroed by the caller) */
enum { DEVMAT_BAD_ROW = 0, DEVMAT_BAD_COL, DEVMAT_BAD_VAL, DEVMAT_NOT_ONE, DEVMAT_HIGH, DEVMAT_COUNTS };

/* a slab is packed with at most this many distinct values; the palette pass stops counting above it */
#define DEVMAT_PAL_MAX 256
/* slots of the palette's hash tables (u64 keys lo | hi << 32; DEVMAT_PAL_EMPTY is no residue below 2^62) */
#define DEVMAT_PAL_SLOTS 1024
#define DEVMAT_PAL_EMPTY 0xFFFFFFFFFFFFFFFFull

/* One pass over the nnz triplets (idx_bytes 4: int32 indices, 8: int64; val_bytes 0: no values, 4: u32, 8: u64):
 * counts[] += the entries with a row outside [0, nrows), a column outside [0, ncols), a value not below p, a value that is
 * not 1, a value of 2^32 or more; cnt0[i]++ / cnt1[j]++ for every index that IS inside (cnt0: nrows + 1 words, cnt1:
 * ncols + 1, zeroed by the caller) -- an index is checked before it is used as an address. */
hipError_t launch_devmat_count(const KernelCfg &c, int idx_bytes, int val_bytes, const void *i, const void *j, const void *x,
			       long long nnz, long long nrows, long long ncols, u32 *cnt0, u32 *cnt1, unsigned long long *counts,
			       hipStream_t s);

/* tile sums the scan of `len` counters needs (words of u32) */
long long devmat_scan_tiles(long long len);
/* a[k] <- a[0] + ... + a[k-1] in place, k < len (sums below 2^32); sums: devmat_scan_tiles(len) words.  Three launches. */
hipError_t launch_devmat_scan(u32 *a, long long len, u32 *sums, hipStream_t s);

/* entry k goes to slot cur0[i]++ of CSR(M) (col0 = j, val0 / hi0 = the limbs of x where those are not NULL) and to slot
 * cur1[j]++ of CSR(M^T); cur0 / cur1: copies of the two row_ptr arrays.  An entry whose index is out of range, or whose slot
 * is not below nnz, is skipped (the caller has read the counts as zero: this only keeps a changed array from faulting). */
hipError_t launch_devmat_scatter(const KernelCfg &c, int idx_bytes, int val_bytes, const void *i, const void *j, const void *x,
				 long long nnz, long long nrows, long long ncols, u32 *cur0, u32 *cur1, int *col0, u32 *val0, u32 *hi0,
				 int *col1, u32 *val1, u32 *hi1, hipStream_t s);

/* distinct values of a slab (hi == NULL: the high limbs are zero): table = DEVMAT_PAL_SLOTS keys set to DEVMAT_PAL_EMPTY and
 * *count = 0 by the caller; afterwards *count > DEVMAT_PAL_MAX means more than that many, else keys[0 .. *count) hold them in
 * no particular order (keys: DEVMAT_PAL_MAX words). */
hipError_t launch_devmat_palette(const KernelCfg &c, const u32 *val, const u32 *hi, long long nnz, unsigned long long *table,
				 unsigned int *count, unsigned long long *keys, hipStream_t s);

/* col[k] |= (index of val[k] | hi[k] << 32 among the nkeys ascending keys) << 24 */
hipError_t launch_devmat_pack(const KernelCfg &c, int *col, const u32 *val, const u32 *hi, long long nnz,
			      const unsigned long long *keys, int nkeys, hipStream_t s);

#endif
