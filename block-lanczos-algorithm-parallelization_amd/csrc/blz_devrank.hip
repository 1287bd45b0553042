/*
 * blz_devrank.hip -- device blocks on several ranks: the bridges between a whole block (every row, the
 * file's numbering) and a rank-local one (the rank's own rows, in the order its slab has), and the last step of an inner
 * product whose sum runs over ranks.
 *
 * Layout walk, as in blz_devio.hip.  Both row kernels walk the LOCAL rows in order: a lane group of L = the next power of two
 * >= the row's units takes one local row, 256 / L consecutive rows per workgroup, so a wavefront's accesses to the local block
 * are one contiguous run where its stride is n.  The whole block's side is row inv[first + q] -- a gather (take) or a scatter
 * (put) of whole rows, each row one contiguous run, the rows wherever the renumbering put them.  A unit is one 8-byte word,
 * or two of them (16-byte lane accesses) where both sides allow it: n even, both strides even, both bases 16-byte aligned.
 * Both sides are the caller's u64 words: the word width in HBM and the padded width of a slab never show here.
 */
#include "blz_devrank.h"

namespace {

constexpr int BLOCK = 256;

/* TAKE: local <- whole, else whole <- local.  Row q of `local` is row id(q) of `whole`; a lane touches words [0, n) only. */
template <bool VEC2, bool TAKE>
__global__ void __launch_bounds__(BLOCK) k_rows_move(u64 *__restrict__ local, long long ldl, u64 *__restrict__ whole, long long ldw,
						      const int *__restrict__ inv, long long first, long long rows, int n, int lg)
{
	const int lane = threadIdx.x & ((1 << lg) - 1), rpb = BLOCK >> lg;
	if (lane >= (VEC2 ? n >> 1 : n))
		return;
	for (long long q = (long long)blockIdx.x * rpb + (threadIdx.x >> lg); q < rows; q += (long long)gridDim.x * rpb) {
		const long long o = inv ? (long long)inv[first + q] : first + q;
		if constexpr (VEC2) {
			ulonglong2 *l = reinterpret_cast<ulonglong2 *>(local + q * ldl + 2 * lane);
			ulonglong2 *w = reinterpret_cast<ulonglong2 *>(whole + o * ldw + 2 * lane);
			if (TAKE)
				*l = *w;
			else
				*w = *l;
		} else {
			if (TAKE)
				local[q * ldl + lane] = whole[o * ldw + lane];
			else
				whole[o * ldw + lane] = local[q * ldl + lane];
		}
	}
}

/* one workgroup per 256 words; at most 2 * 64 * 64 of them */
__global__ void __launch_bounds__(BLOCK) k_residue_sums(u64 *__restrict__ out, const u64 *__restrict__ sums, int words, u64 p)
{
	const int i = blockIdx.x * BLOCK + threadIdx.x;
	if (i < words)
		out[i] = sums[i] % p;
}

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

inline bool pair_ok(const void *a, long long lda, const void *b, long long ldb, int n)
{
	return (n & 1) == 0 && (lda & 1) == 0 && (ldb & 1) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

template <bool TAKE>
hipError_t rows_move(const KernelCfg &c, u64 *local, long long ldl, u64 *whole, long long ldw, const int *inv, long long first,
		     long long rows, int n, hipStream_t s)
{
	if (rows <= 0)
		return hipSuccess;
	const bool v2 = pair_ok(local, ldl, whole, ldw, n);
	const Shape sh = shape_for(c, rows, v2 ? n / 2 : n);
	if (v2)
		hipLaunchKernelGGL((k_rows_move<true, TAKE>), dim3(sh.grid), dim3(BLOCK), 0, s, local, ldl, whole, ldw, inv, first, rows, n,
				   sh.lg);
	else
		hipLaunchKernelGGL((k_rows_move<false, TAKE>), dim3(sh.grid), dim3(BLOCK), 0, s, local, ldl, whole, ldw, inv, first, rows, n,
				   sh.lg);
	return hipGetLastError();
}

}  // namespace

hipError_t launch_rows_take(const KernelCfg &c, u64 *local, long long ldl, const u64 *whole, long long ldw, const int *inv,
			    long long first, long long rows, int n, hipStream_t s)
{
	return rows_move<true>(c, local, ldl, const_cast<u64 *>(whole), ldw, inv, first, rows, n, s);
}

hipError_t launch_rows_put(const KernelCfg &c, u64 *whole, long long ldw, const u64 *local, long long ldl, const int *inv,
			   long long first, long long rows, int n, hipStream_t s)
{
	return rows_move<false>(c, const_cast<u64 *>(local), ldl, whole, ldw, inv, first, rows, n, s);
}

hipError_t launch_residue_sums(const KernelCfg &c, u64 *out, const u64 *sums, int words, hipStream_t s)
{
	if (words <= 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_residue_sums, dim3((unsigned)((words + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, out, sums, words, c.m.p);
	return hipGetLastError();
}
