/* blz_devsmall.h -- launchers of the device small algebra kernels (blz_devsmall.hip): the n x n chain between the inner
 * product and the recombination of a Krylov step (semi-inverse, step coefficients) and the reduced row echelon form of a
 * caller's block, all on u64 words in device memory, whatever the context's word size.  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVSMALL_H
#define BLZ_DEVSMALL_H

#include "blz_kernels.h"

#define DEVSMALL_COEF_PANELS 5	/* = BLZ_COEF_PANELS of blz.h; the panel order is that of its enum */

/* semi_inverse() of sequential/lanczos_modp.c:342-438 on the n x n residues `vtav`, one workgroup, one launch.
 *   coef == nullptr: winv (n x n) and d (n words, 0 or 1) are written.
 *   coef != nullptr: vtaav (n x n) is read as well and the five n x n panels of orthogonalize() (:456-475) are written to
 *                    coef -- D, (I - D) - W * S, -vtav * D, I - D, W -- and neither winv nor d.
 * npiv (one word, may be nullptr) = the pivot count.  n is the caller's width (1 .. 64); of c only the modulus and its
 * reducer class are read.  No output may overlap an input or another output (the caller has checked). */
hipError_t launch_dev_chain(const KernelCfg &c, int n, const u64 *vtav, const u64 *vtaav, u64 *winv, u64 *d, u64 *coef, u64 *npiv,
			    hipStream_t s);

/* Canonical RREF of the row space of x (rows x n u64 words, row stride ldx >= n, any rows >= 0): two launches.
 * The partial launch appends every workgroup's echelon rows to `stack` (room for dev_rref_stack_rows() rows of n words) and
 * stops reading once a workgroup has reached rank n; ctl[0] = rank-n flag, ctl[1] = rows stacked, both zeroed here on the
 * stream.  The merge launch (one workgroup) writes e (n x n, rows sorted by pivot column, zero from the rank on), info
 * (n + 1 int64 words: the rank, then the pivot column of row i, -1 from the rank on) and, when z != nullptr, the canonical
 * null basis of e (n x n: column jj for the jj-th free column f has 1 at f and -e[i][f] at pivot i; zero columns from
 * n - rank on). */
long long dev_rref_stack_rows(const KernelCfg &c, int n);
hipError_t launch_dev_rref(const KernelCfg &c, int n, long long rows, const u64 *x, long long ldx, u64 *stack, int *ctl, u64 *e,
			   u64 *z, long long *info, hipStream_t s);

#endif
