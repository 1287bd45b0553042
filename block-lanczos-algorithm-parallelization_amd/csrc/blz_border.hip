/*
 * blz_border.hip -- the dense 64-bit border of the operator M' = [M | b] (M x = b) resp. [M ; b] (x M = b).
 *
 * The matrix itself carries one extra EMPTY row / column (its values are u32 and cannot hold b); b lives on the device
 * as one word per row of side 1 (the rows of tmp), in the solver's numbering.  Two streaming kernels behind the products:
 *   k_border_update   tmp[r, :] += b[r] * v[border, :]          after the product that writes side 1
 *   k_border_dot      Av[border, :] = sum_r b[r] * tmp[r, :]    after the product that writes side 0 (partial rows per
 *                     workgroup, k_border_finalize sums them and stores the row in the slab's word width)
 * Both are no-ops once the stop flag is up, like the products they follow.  Exact for every 2 <= p < 2^62: one
 * 128-bit (96-bit for 32-bit words) sum per output word, reduced with the reducers of modp.h, at most m.chunk
 * products between two reductions.
 */
#include "blz_border.h"

#include <type_traits>

#define BLOCK 256

template <typename W, int VEC>
struct alignas(sizeof(W) * VEC) WordVec {
	W w[VEC];
};

/* (x + b * v) mod p for residues of the context's width */
template <typename W, int MERS>
__device__ __forceinline__ W border_fma(u64 x, u64 b, u64 v, const ModP &m)
{
	if (sizeof(W) == 4) {
		const u64 t = b * v + x;	/* b, v, x < 2^32: below 2^64 */
		return (W)reduce128<MERS>(0, t, m);
	}
	const unsigned __int128 t = (unsigned __int128)b * v + x;	/* < p^2 + p < 2^(63 + k) */
	return (W)reduce128<MERS>((u64)(t >> 64), (u64)t, m);
}

/*
 * T[r, j] = (T[r, j] + B[r] * vb[j]) mod p, rows x n words, VEC words (16 bytes when n allows) per lane and step.
 * vb = the n words of the border row of the operand block, read from the device (no host trip) into LDS once per
 * workgroup.  Bytes: one read and one write of T, one read of B.
 */
template <typename W, int MERS, int VEC, bool POW2>
__global__ void __launch_bounds__(BLOCK)
k_border_update(W *__restrict__ T, const W *__restrict__ B, const W *__restrict__ vb, long long rows, int n, int sh,
		ModP m, const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	__shared__ u64 vs[BLZ_BORDER_MAXN];
	if (threadIdx.x < BLZ_BORDER_MAXN)
		vs[threadIdx.x] = (int)threadIdx.x < n ? (u64)vb[threadIdx.x] : 0;
	__syncthreads();
	using Vec = WordVec<W, VEC>;
	Vec *__restrict__ T4 = (Vec *)T;
	const long long total = rows * n / VEC, step = (long long)gridDim.x * BLOCK;
	for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < total; q += step) {
		const long long e = q * VEC;
		const long long r = POW2 ? (e >> sh) : (e / n);
		const int j = (int)(e - r * n);
		const u64 b = B[r];
		Vec x = T4[q];
#pragma unroll
		for (int u = 0; u < VEC; u++)
			x.w[u] = border_fma<W, MERS>(x.w[u], b, vs[j + u], m);
		T4[q] = x;
	}
}

/*
 * partial[block][col] = sum over the block's rows of B[r] * T[r, col] mod p.  A lane is (row of the wavefront, column): G =
 * the width rounded up to a power of two (= the width in the padded layout), 64 / G rows per wavefront and load, four
 * rows per lane in flight.  Bytes: one read of T, one read of B.
 */
template <typename W, int MERS>
__global__ void __launch_bounds__(BLOCK)
k_border_dot(const W *__restrict__ T, const W *__restrict__ B, long long rows, int n, int G, ModP m,
	     u64 *__restrict__ partial, const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	constexpr int U = 4;
	using A = typename std::conditional<sizeof(W) == 4, AccS, Acc>::type;
	__shared__ u64 red[BLOCK / 64][BLZ_BORDER_MAXN];
	const int t = threadIdx.x, lane = t & 63, col = lane & (G - 1), gpb = BLOCK / G;
	const bool mine = col < n;
	const long long g0 = (long long)blockIdx.x * gpb + t / G, ng = (long long)gridDim.x * gpb;
	A acc;
	acc_zero(acc);
	u32 cnt = 0;
	for (long long r = g0; r < rows; r += ng * U) {
		u64 x[U], b[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			const long long rr = r + u * ng;
			const bool ok = mine && rr < rows;
			x[u] = ok ? (u64)T[rr * n + col] : 0;
			b[u] = ok ? (u64)B[rr] : 0;
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
			acc_mac64(acc, b[u], x[u]);
			if (++cnt == m.chunk) {
				cnt = 0;
				acc_set(acc, acc_reduce<MERS>(acc, m));
			}
		}
	}
	u64 s = acc_reduce<MERS>(acc, m);
	for (int off = G; off < 64; off <<= 1)
		s = addmod(s, (u64)__shfl_xor((unsigned long long)s, off, 64), m.p);
	if (lane < G)
		red[t >> 6][lane] = s;
	__syncthreads();
	if (t < G) {
		u64 x = 0;
#pragma unroll
		for (int w = 0; w < BLOCK / 64; w++)
			x = addmod(x, red[w][t], m.p);
		partial[(size_t)blockIdx.x * G + t] = x;
	}
}

/* out[col] = sum_b partial[b][col] mod p, stored in the slab's word width: one workgroup, BLOCK / G lanes per column */
template <typename W>
__global__ void __launch_bounds__(BLOCK)
k_border_finalize(const u64 *__restrict__ partial, int nblocks, int n, int G, u64 p, W *__restrict__ out,
		  const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	__shared__ u64 red[BLOCK];
	const int t = threadIdx.x, col = t & (G - 1), part = t / G, parts = BLOCK / G;
	u64 s = 0;
	for (int b = part; b < nblocks; b += parts)
		s = addmod(s, partial[(size_t)b * G + col], p);
	red[t] = s;
	__syncthreads();
	if (t < G && t < n) {
		u64 x = 0;
		for (int q = 0; q < parts; q++)
			x = addmod(x, red[q * G + t], p);
		out[t] = (W)x;
	}
}

static inline int border_group(int n)
{
	int G = 1;
	while (G < n)
		G <<= 1;
	return G;
}

int border_dot_max_blocks(const KernelCfg &c) { return c.num_cu * 8; }

template <typename W, int MERS>
static void border_update_go(const KernelCfg &c, W *T, const W *B, const W *vb, long long rows, const DevCtl *ctl, hipStream_t s)
{
	constexpr int V16 = 16 / (int)sizeof(W);
	const int n = c.n;
	const bool pow2 = (n & (n - 1)) == 0;
	int sh = 0;
	while ((1 << sh) < n)
		sh++;
	const bool wide = n % V16 == 0;
	const long long total = rows * n / (wide ? V16 : 1);
	long long blocks = (total + BLOCK - 1) / BLOCK;
	blocks = blocks < 1 ? 1 : (blocks > (long long)c.num_cu * 8 ? (long long)c.num_cu * 8 : blocks);
	const dim3 grid((unsigned)blocks), blk(BLOCK);
	if (wide && pow2)
		hipLaunchKernelGGL((k_border_update<W, MERS, V16, true>), grid, blk, 0, s, T, B, vb, rows, n, sh, c.m, ctl);
	else if (wide)
		hipLaunchKernelGGL((k_border_update<W, MERS, V16, false>), grid, blk, 0, s, T, B, vb, rows, n, sh, c.m, ctl);
	else if (pow2)
		hipLaunchKernelGGL((k_border_update<W, MERS, 1, true>), grid, blk, 0, s, T, B, vb, rows, n, sh, c.m, ctl);
	else
		hipLaunchKernelGGL((k_border_update<W, MERS, 1, false>), grid, blk, 0, s, T, B, vb, rows, n, sh, c.m, ctl);
}

hipError_t launch_border_update(const KernelCfg &c, void *T, const void *B, const void *vb, int64_t rows, const DevCtl *ctl,
				hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN)
		return hipErrorInvalidValue;
	if (rows <= 0)
		return hipSuccess;
	if (c.word == 4) {
		if (c.mers == 31)
			border_update_go<u32, 31>(c, (u32 *)T, (const u32 *)B, (const u32 *)vb, rows, ctl, s);
		else
			border_update_go<u32, 0>(c, (u32 *)T, (const u32 *)B, (const u32 *)vb, rows, ctl, s);
	} else {
		if (c.mers == 61)
			border_update_go<u64, 61>(c, (u64 *)T, (const u64 *)B, (const u64 *)vb, rows, ctl, s);
		else
			border_update_go<u64, 0>(c, (u64 *)T, (const u64 *)B, (const u64 *)vb, rows, ctl, s);
	}
	return hipGetLastError();
}

hipError_t launch_border_dot(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *out_row,
			     const DevCtl *ctl, hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN)
		return hipErrorInvalidValue;
	const int n = c.n, G = border_group(n), gpb = BLOCK / G;
	long long blocks = (rows + (long long)gpb * 4 - 1) / ((long long)gpb * 4);
	blocks = blocks < 1 ? 1 : (blocks > border_dot_max_blocks(c) ? border_dot_max_blocks(c) : blocks);
	const dim3 grid((unsigned)blocks), blk(BLOCK);
	if (c.word == 4) {
		if (c.mers == 31)
			hipLaunchKernelGGL((k_border_dot<u32, 31>), grid, blk, 0, s, (const u32 *)T, (const u32 *)B, (long long)rows, n, G, c.m,
					   partial, ctl);
		else
			hipLaunchKernelGGL((k_border_dot<u32, 0>), grid, blk, 0, s, (const u32 *)T, (const u32 *)B, (long long)rows, n, G, c.m,
					   partial, ctl);
		hipLaunchKernelGGL((k_border_finalize<u32>), dim3(1), blk, 0, s, partial, (int)blocks, n, G, c.m.p, (u32 *)out_row, ctl);
	} else {
		if (c.mers == 61)
			hipLaunchKernelGGL((k_border_dot<u64, 61>), grid, blk, 0, s, (const u64 *)T, (const u64 *)B, (long long)rows, n, G, c.m,
					   partial, ctl);
		else
			hipLaunchKernelGGL((k_border_dot<u64, 0>), grid, blk, 0, s, (const u64 *)T, (const u64 *)B, (long long)rows, n, G, c.m,
					   partial, ctl);
		hipLaunchKernelGGL((k_border_finalize<u64>), dim3(1), blk, 0, s, partial, (int)blocks, n, G, c.m.p, (u64 *)out_row, ctl);
	}
	return hipGetLastError();
}
