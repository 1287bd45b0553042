/* blz_devw32.h -- launchers of the 32-bit device-block kernels (blz_devw32.hip): the device-block family on a caller's blocks
 * of uint32_t words -- rows x n residues below p < 2^32, row stride ld counted in 32-bit words, the words n .. ld-1 of a row
 * never read or written.  The n x n operands (results of the inner products, coefficients of the recombinations) are
 * contiguous u64 words, as in blz_devalg.h.  Only contexts of 4-byte words (c.word == 4) come here.
 * C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVW32_H
#define BLZ_DEVW32_H

#include "blz_devalg.h"

/* 32-bit words a lane moves per access of a caller's block: 4 (16 bytes), 2 (8 bytes) or 1 (4 bytes).  The pointer, the
 * stride and the width must all allow it: n and ld multiples of the width, the base aligned to the width's bytes.  A call
 * runs at the least width of its blocks.  (tests/device_w32_ref.py restates this and the tile sizes below.) */
int dev_w32_width(const void *block, long long ld, int n);

/* rows of a tile of the inner products at width n: W32_TILE_WORDS >> ceil(log2 n) */
#define W32_TILE_WORDS 2048
int dev_w32_tile_rows(int n);

/* slab[s][0..np) <- caller[inv[s]][0..un), columns un..np-1 zero, s in [0, rows); slab: u32 words, np = c.n per row.
 * inv == nullptr: the identity.  bad != nullptr: *bad += the caller's words that are not below c.m.p. */
hipError_t launch_w32_import(const KernelCfg &c, void *slab, const u32 *caller, long long ld, const int *inv, long long rows,
			     int un, unsigned long long *bad, hipStream_t s);
/* caller[inv[s]][0..un) <- slab[s][0..un); words un..ld-1 of a caller's row are not written */
hipError_t launch_w32_export(const KernelCfg &c, u32 *caller, long long ld, const void *slab, const int *inv, long long rows,
			     int un, hipStream_t s);

/* out[k * n * n + i * n + j] = sum_r x[k][r * ldx[k] + i] * y[r * ldy + j] mod p for k < nx, nx = 1 (blz_dot_device32) or 2
 * (blz_dot_pair_device32).  Blocks that are the same pointer with the same stride are staged once (dev_same_blocks).  Every
 * workgroup writes ONE row of nx * n * n canonical u64 residues to `partial` -- room for dev_dot_max_blocks() rows of them: the
 * scratch of the 64-bit namesakes -- and launch_dev_dot_finalize adds the rows mod p into `out`.  rows == 0: out = 0. */
hipError_t launch_w32_dot(const KernelCfg &c, int n, long long rows, int nx, const u32 *const *x, const long long *ldx,
			  const u32 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s);

/* z[o][r * ldz[o] + j] = sum_t sum_i x[t][r * ldx[t] + i] * a[o][t][i * n + j] mod p over the terms with a[o][t] != NULL,
 * o < nz, nz = 1 (blz_combine_device32) or 2 (blz_combine_pair_device32); 1 <= nterms <= DEVALG_MAX_TERMS.  ONE launch at
 * every width and term count.  A lane group reads its row of every term before it stores: each z[o] may BE one of the x[t]
 * (same pointer, same stride). */
hipError_t launch_w32_combine(const KernelCfg &c, int n, long long rows, int nterms, const u32 *const *x, const long long *ldx,
			      int nz, const u64 *const *a0, const u64 *const *a1, u32 *z0, long long ldz0, u32 *z1, long long ldz1,
			      hipStream_t s);

#endif
