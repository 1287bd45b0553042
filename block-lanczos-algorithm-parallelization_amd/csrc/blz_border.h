/* blz_border.h -- launchers of the border kernels of a solve with a right-hand side (blz_border.hip; C++ side only). */
#ifndef BLZ_BORDER_H
#define BLZ_BORDER_H

#include "blz_kernels.h"

/* B = one word of the context's width per row of T (the right-hand side, in the solver's numbering of side 1).
 * launch_border_update: T[r, :] = (T[r, :] + B[r] * vb[:]) mod p, rows x c.n words; vb = the c.n words of the border row of
 * the operand block, on the device.
 * launch_border_dot: out_row[:] = sum_r B[r] * T[r, :] mod p (c.n words of the context's width); partial = room for
 * border_dot_max_blocks(c) * BLZ_BORDER_MAXN u64 words.
 * Both are no-ops once the stop flag is up, like the products they follow. */
#define BLZ_BORDER_MAXN 64
int border_dot_max_blocks(const KernelCfg &c);
hipError_t launch_border_update(const KernelCfg &c, void *T, const void *B, const void *vb, int64_t rows, const DevCtl *ctl,
				hipStream_t s);
hipError_t launch_border_dot(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *out_row,
			     const DevCtl *ctl, hipStream_t s);

#endif
