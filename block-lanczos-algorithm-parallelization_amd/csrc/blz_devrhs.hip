/*
 * blz_devrhs.hip -- device right-hand sides: the two ends of M x = b on caller-owned device memory.
 *
 *   k_rhs_import        the border of the bordered operator from b: what blz_set_rhs / blz_set_rhs_block do on the host with
 *                       a permuting loop and an upload
 *   k_solution_export   the k solution columns of V into x: what blz_solution_block does with a copy of the whole block to
 *                       the host and a loop over its rows
 *
 * Layout walk.  Both are one streaming pass with a gather / scatter of short rows on the caller's side only.  A lane takes one
 * (row, column) of the SLAB side, flat: lane t of the grid works on slab row t >> lg, column t & (2^lg - 1), with 2^lg the
 * words per row of the border (import: kp, a power of two, or 1) or the next power of two >= k (export).  So a wavefront's
 * slab accesses are one contiguous run (import: 64 consecutive words of the border; export: 2^lg of every c.n words of V),
 * and the caller's side is row inv[s], k contiguous words wherever the renumbering put them -- the same price the device
 * blocks pay (blz_devio.hip).  Grid-stride over the flat index; plain stores.
 */
#include "blz_devrhs.h"
#include "blz_devhelp.h"

namespace {

constexpr int BLOCK = 256;

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
	for (int off = 32; off > 0; off >>= 1)
		v += __shfl_xor(v, off, 64);
	return v;
}

/* S: the border's word, W: the caller's.  The words that are not below p are counted, one atomic per wavefront that saw any */
template <typename S, typename W>
__global__ void __launch_bounds__(BLOCK) k_rhs_import(S *__restrict__ rhs, const W *__restrict__ b, long long ldb,
						       const int *__restrict__ inv, long long rows, int k, int lg, u64 p,
						       unsigned long long *bad)
{
	const long long total = rows << lg;
	unsigned long long cnt = 0;
	for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BLOCK) {
		const long long s = t >> lg;
		const int i = (int)(t & ((1 << lg) - 1));
		u64 v = 0;
		if (i < k) {
			const long long o = inv ? (long long)inv[s] : s;
			v = (u64)b[o * ldb + i];
			cnt += v >= p;
		}
		rhs[t] = (S)v;
	}
	cnt = wave_sum(cnt);
	if ((threadIdx.x & 63) == 0 && cnt)
		atomicAdd(bad, cnt);
}

template <typename S, typename W>
__global__ void __launch_bounds__(BLOCK) k_solution_export(W *__restrict__ x, long long ldx, const S *__restrict__ V,
							    const int *__restrict__ inv, long long rows, long long xrows, int k,
							    int np, int lg)
{
	const long long total = rows << lg;
	for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BLOCK) {
		const long long s = t >> lg;
		const int j = (int)(t & ((1 << lg) - 1));
		if (j >= k)
			continue;
		const long long o = inv ? (long long)inv[s] : s;
		if (o < xrows)		/* (the border rows are the last k of the original numbering) */
			x[o * ldx + j] = (W)V[s * np + j];
	}
}

/* every CU a few workgroups, the rest of the flat index by the grid stride */
inline unsigned grid_for(const KernelCfg &c, long long total)
{
	const long long want = (total + BLOCK - 1) / BLOCK, cap = (long long)c.num_cu * 8;
	return (unsigned)(want < cap ? want : cap);
}

}  // namespace

template <typename W>
hipError_t launch_rhs_import(const KernelCfg &c, void *rhs, const W *b, long long ldb, const int *inv, long long rows, int k,
			     int kp, unsigned long long *bad, hipStream_t s)
{
	if (rows <= 0)
		return hipSuccess;
	const int kw = kp > 0 ? kp : 1;
	if (k < 1 || k > kw || (kw & (kw - 1)) != 0 || ldb < k || !bad)
		return hipErrorInvalidValue;
	const int lg = log2_ceil(kw);
	const unsigned grid = grid_for(c, rows << lg);
	if (c.word == 4)
		hipLaunchKernelGGL((k_rhs_import<u32, W>), dim3(grid), dim3(BLOCK), 0, s, (u32 *)rhs, b, ldb, inv, rows, k, lg, c.m.p, bad);
	else
		hipLaunchKernelGGL((k_rhs_import<u64, W>), dim3(grid), dim3(BLOCK), 0, s, (u64 *)rhs, b, ldb, inv, rows, k, lg, c.m.p, bad);
	return hipGetLastError();
}

template <typename W>
hipError_t launch_solution_export(const KernelCfg &c, W *x, long long ldx, const void *V, const int *inv, long long rows,
				  long long xrows, int k, hipStream_t s)
{
	if (rows <= 0 || xrows <= 0)
		return hipSuccess;
	if (k < 1 || k > c.n || ldx < k || xrows > rows)
		return hipErrorInvalidValue;
	if (c.word == 8 && sizeof(W) == 4)
		return hipErrorInvalidValue;	/* residues of an 8-byte slab do not fit the caller's word */
	const int lg = log2_ceil(k);
	const unsigned grid = grid_for(c, rows << lg);
	if (c.word == 4)
		hipLaunchKernelGGL((k_solution_export<u32, W>), dim3(grid), dim3(BLOCK), 0, s, x, ldx, (const u32 *)V, inv, rows, xrows,
				   k, c.n, lg);
	else
		hipLaunchKernelGGL((k_solution_export<u64, W>), dim3(grid), dim3(BLOCK), 0, s, x, ldx, (const u64 *)V, inv, rows, xrows,
				   k, c.n, lg);
	return hipGetLastError();
}

#define DEVRHS_INSTANCES(X) X(u64) X(u32)
#define X(W)                                                                                                                     \
	template hipError_t launch_rhs_import<W>(const KernelCfg &, void *, const W *, long long, const int *, long long, int, int, \
						 unsigned long long *, hipStream_t);                                             \
	template hipError_t launch_solution_export<W>(const KernelCfg &, W *, long long, const void *, const int *, long long,     \
						      long long, int, hipStream_t);
DEVRHS_INSTANCES(X)
#undef X
