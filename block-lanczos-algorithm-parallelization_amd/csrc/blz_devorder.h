/* blz_devorder.h -- launchers of the device renumbering (blz_devorder.hip): blz_reorder's order -- rows by smallest column,
 * columns by smallest new row, ties in ascending original index -- made on the GPU from a caller's triplets, and the
 * relabelled int32 triplets that blz_devmat.hip then builds both CSRs from (blz_set_matrix_device_ordered /
 * blz_set_matrix_upload_ordered).  Passes are ordered by kernel boundaries alone.
 * C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVORDER_H
#define BLZ_DEVORDER_H

#include "blz_kernels.h"

/* the stable sort: least significant digit first, DEVORDER_DIGIT_BITS bits a pass, a workgroup takes DEVORDER_SORT_TILE items
 * (tests/device_order_ref.py restates both) */
#define DEVORDER_SORT_TILE 256
#define DEVORDER_DIGIT_BITS 8
#define DEVORDER_DIGITS (1 << DEVORDER_DIGIT_BITS)

/* key[0 .. count) <- value */
hipError_t launch_devorder_fill(const KernelCfg &c, int32_t *key, long long count, int32_t value, hipStream_t s);

/* One pass over the nnz triplets (idx_bytes 4: int32 indices, 8: int64), entries with BOTH indices inside only:
 * by_col == 0:  key[i] <- min(key[i], j)             (key: nrows words; perm is not read)
 * by_col != 0:  key[j] <- min(key[j], perm[i])       (key: ncols words; perm: nrows words, the new index of every row)
 * An index is compared with its bound before it is used as an address. */
hipError_t launch_devorder_min(const KernelCfg &c, int idx_bytes, const void *i, const void *j, long long nnz, long long nrows,
			       long long ncols, const int32_t *perm, int32_t *key, int by_col, hipStream_t s);

/* digit passes of a sort of keys in [0, nkeys]: ceil(bits(nkeys) / DEVORDER_DIGIT_BITS) */
int devorder_sort_passes(long long nkeys);
/* what the sort of `count` items needs besides key and perm: words (4 bytes each) of each of the four ping-pong buffers, of
 * the digit-major count matrix, and of the tile sums of its scan */
long long devorder_sort_tiles(long long count);
long long devorder_sort_counters(long long count);

/* Stable sort of `count` items by key[item] in [0, nkeys]: perm[item] = position.  Items with equal keys keep their order.
 * buf_key[2] / buf_item[2]: `count` words each; counters: devorder_sort_counters(count) words; sums: the tile sums
 * launch_devmat_scan wants for that many counters.  key is only read.  Every pass is three steps -- per-tile digit counts,
 * one exclusive scan of the digit-major count matrix (launch_devmat_scan), a scatter in which an item's rank inside its
 * tile is the number of earlier items of the tile with the same digit -- and no workgroup waits for another. */
hipError_t launch_devorder_sort(const KernelCfg &c, const int32_t *key, long long count, long long nkeys, int32_t *perm,
				int32_t *const buf_key[2], int32_t *const buf_item[2], u32 *counters, u32 *sums, hipStream_t s);

/* ni[k] = row_perm[i[k]], nj[k] = col_perm[j[k]] as int32; an index outside [0, nrows) / [0, ncols) goes through as -1 (and
 * is never used as an address).  ni, nj: nnz words each, 16-byte aligned. */
hipError_t launch_devorder_relabel(const KernelCfg &c, int idx_bytes, const void *i, const void *j, long long nnz,
				   long long nrows, long long ncols, const int32_t *row_perm, const int32_t *col_perm, int32_t *ni,
				   int32_t *nj, hipStream_t s);

#endif
