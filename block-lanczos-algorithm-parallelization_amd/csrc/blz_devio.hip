/*
 * blz_devio.hip -- device blocks: a caller's block that already lives in device memory (rows in the file's numbering, u64
 * words, row stride ld) into a slab of the solver (its own numbering, np words of the context's width per row, the columns
 * past the caller's n zero), and back.  What blz_set_block / blz_get_block do on the host with a copy each way.
 *
 * Layout walk.  Both kernels walk the SLAB rows in order: a lane group of L = the next power of two >= the row's units
 * takes one slab row, 256 / L consecutive rows per workgroup, so a wavefront's accesses to the slab are one contiguous run
 * (64-byte rows at n = 8: 8 rows = 512 bytes per wavefront instruction).  The caller's side is row inv[s] -- a gather (import)
 * or a scatter (export) of whole rows: each row is contiguous, the rows are wherever the renumbering put them.  At n = 8 a
 * 64-byte row costs a 128-byte line fill of which half is used, exactly as a gathered block row in the SpMV (DESIGN.md
 * section 4).  That is the price of the permutation; nothing here tries to hide it.
 * A unit is one 8-byte word, or two of them (16-byte lane accesses) where both sides allow it: un == np even, 8-byte slab
 * words, ld even and a 16-byte aligned base.
 */
#include "blz_devio.h"

namespace {

constexpr int BLOCK = 256;

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
	for (int off = 32; off > 0; off >>= 1)
		v += __shfl_xor(v, off, 64);
	return v;
}

/* COUNT: the words that are not below p are counted, one atomic per wavefront that saw any */
template <typename W, bool VEC2, bool COUNT>
__global__ void __launch_bounds__(BLOCK) k_block_import(W *__restrict__ slab, const u64 *__restrict__ caller, long long ld,
							 const int *__restrict__ inv, long long rows, int un, int np, int lg, u64 p,
							 unsigned long long *bad)
{
	const int lane = threadIdx.x & ((1 << lg) - 1), rpb = BLOCK >> lg;
	const int units = VEC2 ? np >> 1 : np;
	unsigned long long cnt = 0;
	if (lane < units)
		for (long long s = (long long)blockIdx.x * rpb + (threadIdx.x >> lg); s < rows; s += (long long)gridDim.x * rpb) {
			const long long o = inv ? (long long)inv[s] : s;
			if constexpr (VEC2) {
				const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(caller + o * ld + 2 * lane);
				*reinterpret_cast<ulonglong2 *>(slab + s * np + 2 * lane) = v;
				if (COUNT)
					cnt += (v.x >= p) + (v.y >= p);
			} else {
				const u64 v = lane < un ? caller[o * ld + lane] : 0;
				slab[s * np + lane] = (W)v;
				if (COUNT)
					cnt += v >= p;
			}
		}
	if (COUNT) {
		cnt = wave_sum(cnt);
		if ((threadIdx.x & 63) == 0 && cnt)
			atomicAdd(bad, cnt);
	}
}

template <typename W, bool VEC2>
__global__ void __launch_bounds__(BLOCK) k_block_export(u64 *__restrict__ caller, long long ld, const W *__restrict__ slab,
							 const int *__restrict__ inv, long long rows, int un, int np, int lg)
{
	const int lane = threadIdx.x & ((1 << lg) - 1), rpb = BLOCK >> lg;
	if (lane >= (VEC2 ? un >> 1 : un))
		return;
	for (long long s = (long long)blockIdx.x * rpb + (threadIdx.x >> lg); s < rows; s += (long long)gridDim.x * rpb) {
		const long long o = inv ? (long long)inv[s] : s;
		if constexpr (VEC2)
			*reinterpret_cast<ulonglong2 *>(caller + o * ld + 2 * lane) =
				*reinterpret_cast<const ulonglong2 *>(slab + s * np + 2 * lane);
		else
			caller[o * ld + lane] = (u64)slab[s * np + lane];
	}
}

__global__ void __launch_bounds__(BLOCK) k_identity_tail(u64 *tail, int n, int words)
{
	for (int i = blockIdx.x * BLOCK + threadIdx.x; i < words; i += gridDim.x * BLOCK)
		tail[i] = (i < n * n && i / n == i % n) ? 1 : 0;
}

/* lane group of a row (log2) and the grid: every CU a few workgroups, rows beyond them by the grid stride */
struct Shape {
	int lg;
	unsigned grid;
};
inline Shape shape_for(const KernelCfg &c, long long rows, int units)
{
	int lg = 0;
	while ((1 << lg) < units)
		lg++;
	const long long rpb = BLOCK >> lg, want = (rows + rpb - 1) / rpb, cap = (long long)c.num_cu * 8;
	return Shape{ lg, (unsigned)(want < cap ? want : cap) };
}

inline bool pair_ok(const KernelCfg &c, const void *caller, long long ld, int un)
{
	return c.word == 8 && un == c.n && (un & 1) == 0 && (ld & 1) == 0 && ((uintptr_t)caller & 15) == 0;
}

}  // namespace

hipError_t launch_block_import(const KernelCfg &c, void *slab, const u64 *caller, long long ld, const int *inv, long long rows,
			       int un, unsigned long long *bad, hipStream_t s)
{
	if (rows <= 0)
		return hipSuccess;
	const int np = c.n;
	const bool v2 = pair_ok(c, caller, ld, un);
	const Shape sh = shape_for(c, rows, v2 ? np / 2 : np);
#define IMPORT(W, V2, CNT)                                                                                                       \
	hipLaunchKernelGGL((k_block_import<W, V2, CNT>), dim3(sh.grid), dim3(BLOCK), 0, s, (W *)slab, caller, ld, inv, rows, un, np, \
			   sh.lg, c.m.p, bad)
	if (c.word == 4) {
		if (bad)
			IMPORT(u32, false, true);
		else
			IMPORT(u32, false, false);
	} else if (v2) {
		if (bad)
			IMPORT(u64, true, true);
		else
			IMPORT(u64, true, false);
	} else {
		if (bad)
			IMPORT(u64, false, true);
		else
			IMPORT(u64, false, false);
	}
#undef IMPORT
	return hipGetLastError();
}

hipError_t launch_block_export(const KernelCfg &c, u64 *caller, long long ld, const void *slab, const int *inv, long long rows,
			       int un, hipStream_t s)
{
	if (rows <= 0)
		return hipSuccess;
	const int np = c.n;
	const bool v2 = pair_ok(c, caller, ld, un);
	const Shape sh = shape_for(c, rows, v2 ? un / 2 : un);
#define EXPORT(W, V2)                                                                                                    \
	hipLaunchKernelGGL((k_block_export<W, V2>), dim3(sh.grid), dim3(BLOCK), 0, s, caller, ld, (const W *)slab, inv, rows, un, np, \
			   sh.lg)
	if (c.word == 4)
		EXPORT(u32, false);
	else if (v2)
		EXPORT(u64, true);
	else
		EXPORT(u64, false);
#undef EXPORT
	return hipGetLastError();
}

hipError_t launch_identity_tail(u64 *small, int n, hipStream_t s)
{
	const int words = (int)(small_words(n) - small_E(n));
	hipLaunchKernelGGL(k_identity_tail, dim3((unsigned)((words + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, small + small_E(n), n,
			   words);
	return hipGetLastError();
}
