/* blz_devio.h -- launchers of the device-block kernels (blz_devio.hip): a caller's block in device memory, rows in the
 * file's numbering, to and from a slab in the solver's numbering.  C++ side only; not part of the C ABI. */
#ifndef BLZ_DEVIO_H
#define BLZ_DEVIO_H

#include "blz_kernels.h"

/* slab[s][0..np) <- caller[inv[s]][0..un), columns un..np-1 zero, for s in [0, rows).  caller: u64 words, row stride ld
 * (>= un); slab: words of c.word bytes (the low half of a caller's word at 4), np = c.n per row.  inv == nullptr: the
 * identity.  bad != nullptr: *bad += the number of caller's words that are not below c.m.p (device memory, zeroed by the
 * caller on the same stream). */
hipError_t launch_block_import(const KernelCfg &c, void *slab, const u64 *caller, long long ld, const int *inv, long long rows,
			       int un, unsigned long long *bad, hipStream_t s);
/* caller[inv[s]][0..un) <- slab[s][0..un), widened; words un..ld-1 of a caller's row are not written */
hipError_t launch_block_export(const KernelCfg &c, u64 *caller, long long ld, const void *slab, const int *inv, long long rows,
			       int un, hipStream_t s);
/* small[small_E(n) .. small_words(n)) <- [I | 0 | 0 flags]: p is the P block as it stands (explicit_p_state without the host) */
hipError_t launch_identity_tail(u64 *small, int n, hipStream_t s);

#endif
