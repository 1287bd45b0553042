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

/* k > 1 right-hand sides, 2 <= k <= BLZ_BORDER_MAXK: B = rows x border_kp(k) words of the context's width, row-major, zero
 * padded; brow = the k border rows of side 0 in the solver's numbering, on the device.
 * launch_border_update_k: T[r, :] = (T[r, :] + sum_i B[r, i] * V[brow[i], :]) mod p; V = the operand block (side 0).
 * launch_border_dot_k: S[brow[i], :] = sum_r B[r, i] * T[r, :] mod p; S = the destination block (side 0); partial = room for
 * border_dot_max_blocks(c) * border_kp(k) * BLZ_BORDER_MAXN u64 words.
 * One pass over T serves all k.  No-ops once the stop flag is up. */
#define BLZ_BORDER_MAXK 16
int border_kp(int k);
hipError_t launch_border_update_k(const KernelCfg &c, void *T, const void *B, const void *V, const long long *brow, int k,
				  int64_t rows, const DevCtl *ctl, hipStream_t s);
hipError_t launch_border_dot_k(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *S,
			       const long long *brow, int k, const DevCtl *ctl, hipStream_t s);

/* Several ranks (blz_set_rhs_ranks): T and B are the rank's own rows.
 * launch_border_dot_send: send[i * c.n + col] = this rank's share of sum_r B[r, i] * T[r, col] mod p, k x c.n 64-bit words
 * (k == 1: the single-border dot; B as in the forms above), for an all-reduce over the ranks; partial as above.
 * launch_border_place: S[own[i], :] = recv[i, :] mod p in the context's width where own[i] >= 0 (own = k local row numbers on
 * the device, -1 for the rows of other ranks); recv = the all-reduced sums, below nranks * p <= 2^64.
 * Both are no-ops once the stop flag is up.
 * launch_border_rows_send: send[i, :] = V[own[i], :] as 64-bit words, zeros where own[i] < 0 (no stop flag: outside the loop). */
hipError_t launch_border_dot_send(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, u64 *send, int k,
				  const DevCtl *ctl, hipStream_t s);
hipError_t launch_border_place(const KernelCfg &c, const u64 *recv, void *S, const long long *own, int k, const DevCtl *ctl,
			       hipStream_t s);
hipError_t launch_border_rows_send(const KernelCfg &c, const void *V, const long long *own, int k, u64 *send, hipStream_t s);

#endif
