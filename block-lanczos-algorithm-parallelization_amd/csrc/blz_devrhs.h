/* blz_devrhs.h -- launchers of the device right-hand side kernels (blz_devrhs.hip): the border of a
 * bordered solve from a caller's block in device memory, and the solution columns of V into one.  C++ side only; not part of
 * the C ABI.  W is the caller's word (u64, or u32 for the 32-bit family, whose slabs are 4-byte words). */
#ifndef BLZ_DEVRHS_H
#define BLZ_DEVRHS_H

#include "blz_kernels.h"

/* rhs[s][0..kw) <- b[inv[s]][0..k), columns k..kw-1 zero, for s in [0, rows): kw = kp words per row of the border (k > 1), one
 * word per row when kp == 0 (k == 1).  b: row stride ldb (>= k) of W words, original numbering; rhs: words of c.word bytes,
 * solver's numbering.  inv == nullptr: the identity.  *bad += the number of words of b that are not below c.m.p (device memory,
 * zeroed by the caller on the same stream). */
template <typename W>
hipError_t launch_rhs_import(const KernelCfg &c, void *rhs, const W *b, long long ldb, const int *inv, long long rows, int k,
			     int kp, unsigned long long *bad, hipStream_t s);
/* x[inv[s]][0..k) <- V[s][0..k), widened, for the slab rows s in [0, rows) whose original row inv[s] is below xrows (the border
 * rows are the last ones of the original numbering and are skipped).  x: row stride ldx (>= k) of W words, words k..ldx-1 of a
 * row are not written; V: c.n words of c.word bytes per row. */
template <typename W>
hipError_t launch_solution_export(const KernelCfg &c, W *x, long long ldx, const void *V, const int *inv, long long rows,
				  long long xrows, int k, hipStream_t s);

#endif
