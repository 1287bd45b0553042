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
 *
 * With k > 1 right-hand sides (up to 16) B holds kp = k rounded up to a power of two words per row, zero padded, the k
 * border rows of side 0 sit anywhere in the slab (brow[] holds their numbers), and the same two passes serve all k:
 *   k_border_update_k tmp[r, :] += sum_i B[r, i] * v[brow[i], :]        one read and one write of tmp
 *   k_border_dot_k    Av[brow[i], :] = sum_r B[r, i] * tmp[r, :]        one read of tmp, k accumulators per lane
 *                     (k_border_finalize_k sums the partial k x n tiles and scatters the k rows)
 *
 * On several ranks (blz_set_rhs_ranks) a rank holds its own rows of tmp and of B.  The update runs as above on the rank's
 * slab, its border rows read from the gathered operand.  The dot is taken over the rank's rows only:
 *   k_border_finalize_send  send[i, :] = this rank's share of border row i, as 64-bit residues (instead of the scatter)
 *   (all-reduce of the k x n words over the ranks: sums below nranks * p <= 2^64)
 *   k_border_place          Av[own[i], :] = recv[i, :] mod p on the rank that owns border row i (own[i] = its local row, -1
 *                           elsewhere), in the slab's word width
 *   k_border_rows_send      send[i, :] = V[own[i], :] or zeros: the border words of the kernel basis for the same all-reduce
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

/*
 * send[i * n + col] = sum_b partial[b][i][col] mod p, workgroup i serving border row i: k_border_finalize_k with the k rows
 * stored one after the other as 64-bit residues instead of scattered into the slab -- the rank's share of the border dot
 * before the all-reduce over the ranks.  kp = 1 reads k_border_dot's partial rows.  (Partial rows and send buffer are
 * 64-bit words whatever the slab's width.)
 */
__global__ void __launch_bounds__(BLOCK)
k_border_finalize_send(const u64 *__restrict__ partial, int nblocks, int n, int G, int kp, u64 p, u64 *__restrict__ send,
		       const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	__shared__ u64 red[BLOCK];
	const int t = threadIdx.x, col = t & (G - 1), part = t / G, parts = BLOCK / G, i = blockIdx.x;
	u64 s = 0;
	for (int b = part; b < nblocks; b += parts)
		s = addmod(s, partial[((size_t)b * kp + i) * G + col], p);
	red[t] = s;
	__syncthreads();
	if (t < G && t < n) {
		u64 x = 0;
		for (int q = 0; q < parts; q++)
			x = addmod(x, red[q * G + t], p);
		send[(size_t)i * n + t] = x;
	}
}

/*
 * S[own[i] * n + col] = recv[i * n + col] mod p for the border rows this rank owns (own[i] >= 0), all n words of the row in
 * the slab's word width.  recv holds sums of nranks residues, below nranks * p <= 2^64.  One workgroup: k * n <= 1024 words.
 */
template <typename W, int MERS>
__global__ void __launch_bounds__(BLOCK)
k_border_place(const u64 *__restrict__ recv, int k, int n, ModP m, W *__restrict__ S, const long long *__restrict__ own,
	       const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	for (int q = threadIdx.x; q < k * n; q += BLOCK) {
		const int i = q / n;
		const long long r = own[i];
		if (r >= 0)
			S[r * n + (q - i * n)] = (W)reduce128<MERS>(0, recv[q], m);
	}
}

/* send[i * n + col] = V[own[i] * n + col] where this rank owns border row i, zero elsewhere (outside the loop: no stop flag) */
template <typename W>
__global__ void __launch_bounds__(BLOCK)
k_border_rows_send(const W *__restrict__ V, const long long *__restrict__ own, int k, int n, u64 *__restrict__ send)
{
	for (int q = threadIdx.x; q < k * n; q += BLOCK) {
		const int i = q / n;
		const long long r = own[i];
		send[q] = r >= 0 ? (u64)V[r * n + (q - i * n)] : 0;
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
	with_word_reducer(c, [&](auto wt, auto mers) {
		using W = typename decltype(wt)::type;
		border_update_go<W, decltype(mers)::value>(c, (W *)T, (const W *)B, (const W *)vb, rows, ctl, s);
	});
	return hipGetLastError();
}

/* the dot and one of its two finalize forms: the row in the slab's width (out_row), or 64-bit words for the all-reduce (send) */
static hipError_t border_dot_go(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *out_row,
				u64 *send, const DevCtl *ctl, hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN)
		return hipErrorInvalidValue;
	const int n = c.n, G = border_group(n), gpb = BLOCK / G;
	long long blocks = (rows + (long long)gpb * 4 - 1) / ((long long)gpb * 4);
	blocks = blocks < 1 ? 1 : (blocks > border_dot_max_blocks(c) ? border_dot_max_blocks(c) : blocks);
	const dim3 grid((unsigned)blocks), blk(BLOCK);
	with_word_reducer(c, [&](auto wt, auto mers) {
		using W = typename decltype(wt)::type;
		hipLaunchKernelGGL((k_border_dot<W, decltype(mers)::value>), grid, blk, 0, s, (const W *)T, (const W *)B, (long long)rows, n, G,
				   c.m, partial, ctl);
		if (!send)
			hipLaunchKernelGGL((k_border_finalize<W>), dim3(1), blk, 0, s, partial, (int)blocks, n, G, c.m.p, (W *)out_row, ctl);
	});
	if (send)
		hipLaunchKernelGGL(k_border_finalize_send, dim3(1), blk, 0, s, partial, (int)blocks, n, G, 1, c.m.p, send, ctl);
	return hipGetLastError();
}

hipError_t launch_border_dot(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *out_row,
			     const DevCtl *ctl, hipStream_t s)
{
	return border_dot_go(c, T, B, rows, partial, out_row, nullptr, ctl, s);
}

/* ---- k right-hand sides: B = rows x KP words (KP = k rounded up to a power of two, zero padded) ---- */

/*
 * T[r, j] = (T[r, j] + sum_{i<k} B[r, i] * v[brow[i], j]) mod p.  The k x n words of the border rows of the operand block
 * V are gathered into LDS once per workgroup (rows k..KP-1 are zero, like B's padding); a lane keeps its row of B in
 * registers and one 128-bit (96-bit) sum per word of its 16 bytes of T, reduced after m.chunk products at the latest.
 * Bytes: one read and one write of T, one read of B.
 */
template <typename W, int MERS, int VEC, bool POW2, int KP>
__global__ void __launch_bounds__(BLOCK)
k_border_update_k(W *__restrict__ T, const W *__restrict__ B, const W *__restrict__ V, const long long *__restrict__ brow,
		  int k, long long rows, int n, int sh, ModP m, const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	using A = typename std::conditional<sizeof(W) == 4, AccS, Acc>::type;
	__shared__ u64 vs[KP][BLZ_BORDER_MAXN];
	for (int q = threadIdx.x; q < KP * BLZ_BORDER_MAXN; q += BLOCK) {
		const int i = q / BLZ_BORDER_MAXN, j = q % BLZ_BORDER_MAXN;
		vs[i][j] = (i < k && j < n) ? (u64)V[brow[i] * n + j] : 0;
	}
	__syncthreads();
	using Vec = WordVec<W, VEC>;
	using BVec = WordVec<W, KP>;
	Vec *__restrict__ T4 = (Vec *)T;
	const BVec *__restrict__ B4 = (const BVec *)B;
	const long long total = rows * n / VEC, step = (long long)gridDim.x * BLOCK;
	for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < total; q += step) {
		const long long e = q * VEC;
		const long long r = POW2 ? (e >> sh) : (e / n);
		const int j = (int)(e - r * n);
		const BVec b = B4[r];
		Vec x = T4[q];
		A acc[VEC];
#pragma unroll
		for (int u = 0; u < VEC; u++)
			acc_set(acc[u], (u64)x.w[u]);
		u32 cnt = 0;
#pragma unroll
		for (int i = 0; i < KP; i++) {
#pragma unroll
			for (int u = 0; u < VEC; u++)
				acc_mac64(acc[u], (u64)b.w[i], vs[i][j + u]);
			if (++cnt == m.chunk && i + 1 < KP) {
				cnt = 0;
#pragma unroll
				for (int u = 0; u < VEC; u++)
					acc_set(acc[u], acc_reduce<MERS>(acc[u], m));
			}
		}
#pragma unroll
		for (int u = 0; u < VEC; u++)
			x.w[u] = (W)acc_reduce<MERS>(acc[u], m);
		T4[q] = x;
	}
}

/*
 * partial[block][i][col] = sum over the block's rows of B[r, i] * T[r, col] mod p, i < KP.  Lanes as in k_border_dot; every
 * loaded word of T feeds KP accumulators, so T is read once for all right-hand sides.  Rows in flight per lane shrink
 * as KP grows (the row of B is KP words of registers per row in flight).
 */
template <typename W, int MERS, int KP>
__global__ void __launch_bounds__(BLOCK)
k_border_dot_k(const W *__restrict__ T, const W *__restrict__ B, long long rows, int n, int G, ModP m,
	       u64 *__restrict__ partial, const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	constexpr int U = KP <= 4 ? 4 : (KP == 8 ? 2 : 1);
	using A = typename std::conditional<sizeof(W) == 4, AccS, Acc>::type;
	using BVec = WordVec<W, KP>;
	__shared__ u64 red[BLOCK / 64][BLZ_BORDER_MAXN];
	const BVec *__restrict__ B4 = (const BVec *)B;
	const int t = threadIdx.x, lane = t & 63, col = lane & (G - 1), gpb = BLOCK / G;
	const bool mine = col < n;
	const long long g0 = (long long)blockIdx.x * gpb + t / G, ng = (long long)gridDim.x * gpb;
	A acc[KP];
#pragma unroll
	for (int i = 0; i < KP; i++)
		acc_zero(acc[i]);
	u32 cnt = 0;
	for (long long r = g0; r < rows; r += ng * U) {
		u64 x[U];
		BVec b[U];
#pragma unroll
		for (int u = 0; u < U; u++) {
			const long long rr = r + u * ng;
			const bool ok = mine && rr < rows;
			x[u] = ok ? (u64)T[rr * n + col] : 0;
			b[u] = B4[rr < rows ? rr : 0];	/* (x = 0 makes the row count for nothing) */
		}
#pragma unroll
		for (int u = 0; u < U; u++) {
#pragma unroll
			for (int i = 0; i < KP; i++)
				acc_mac64(acc[i], (u64)b[u].w[i], x[u]);
			if (++cnt == m.chunk) {
				cnt = 0;
#pragma unroll
				for (int i = 0; i < KP; i++)
					acc_set(acc[i], acc_reduce<MERS>(acc[i], m));
			}
		}
	}
#pragma unroll
	for (int i = 0; i < KP; i++) {
		u64 s = acc_reduce<MERS>(acc[i], m);
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
			partial[((size_t)blockIdx.x * KP + i) * G + t] = x;
		}
		__syncthreads();
	}
}

/* S[brow[i] * n + col] = sum_b partial[b][i][col] mod p in the slab's word width: workgroup i serves border row i */
template <typename W>
__global__ void __launch_bounds__(BLOCK)
k_border_finalize_k(const u64 *__restrict__ partial, int nblocks, int n, int G, int kp, u64 p, W *__restrict__ S,
		    const long long *__restrict__ brow, const DevCtl *__restrict__ ctl)
{
	if (ctl->stop)
		return;
	__shared__ u64 red[BLOCK];
	const int t = threadIdx.x, col = t & (G - 1), part = t / G, parts = BLOCK / G, i = blockIdx.x;
	u64 s = 0;
	for (int b = part; b < nblocks; b += parts)
		s = addmod(s, partial[((size_t)b * kp + i) * G + col], p);
	red[t] = s;
	__syncthreads();
	if (t < G && t < n) {
		u64 x = 0;
		for (int q = 0; q < parts; q++)
			x = addmod(x, red[q * G + t], p);
		S[brow[i] * n + t] = (W)x;
	}
}

int border_kp(int k)
{
	int kp = 2;
	while (kp < k)
		kp <<= 1;
	return kp;
}

template <typename W, int MERS, int KP>
static void border_update_k_go(const KernelCfg &c, W *T, const W *B, const W *V, const long long *brow, int k, long long rows,
			       const DevCtl *ctl, hipStream_t s)
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
		hipLaunchKernelGGL((k_border_update_k<W, MERS, V16, true, KP>), grid, blk, 0, s, T, B, V, brow, k, rows, n, sh, c.m, ctl);
	else if (wide)
		hipLaunchKernelGGL((k_border_update_k<W, MERS, V16, false, KP>), grid, blk, 0, s, T, B, V, brow, k, rows, n, sh, c.m, ctl);
	else if (pow2)
		hipLaunchKernelGGL((k_border_update_k<W, MERS, 1, true, KP>), grid, blk, 0, s, T, B, V, brow, k, rows, n, sh, c.m, ctl);
	else
		hipLaunchKernelGGL((k_border_update_k<W, MERS, 1, false, KP>), grid, blk, 0, s, T, B, V, brow, k, rows, n, sh, c.m, ctl);
}

template <typename W, int MERS, int KP>
static void border_dot_k_go(const KernelCfg &c, const W *T, const W *B, long long rows, u64 *partial, W *S, const long long *brow,
			    int k, u64 *send, const DevCtl *ctl, hipStream_t s)
{
	constexpr int U = KP <= 4 ? 4 : (KP == 8 ? 2 : 1);
	const int n = c.n, G = border_group(n), gpb = BLOCK / G;
	long long blocks = (rows + (long long)gpb * U - 1) / ((long long)gpb * U);
	blocks = blocks < 1 ? 1 : (blocks > border_dot_max_blocks(c) ? border_dot_max_blocks(c) : blocks);
	hipLaunchKernelGGL((k_border_dot_k<W, MERS, KP>), dim3((unsigned)blocks), dim3(BLOCK), 0, s, T, B, rows, n, G, c.m, partial, ctl);
	if (send)
		hipLaunchKernelGGL(k_border_finalize_send, dim3((unsigned)k), dim3(BLOCK), 0, s, partial, (int)blocks, n, G, KP, c.m.p,
				   send, ctl);
	else
		hipLaunchKernelGGL((k_border_finalize_k<W>), dim3((unsigned)k), dim3(BLOCK), 0, s, partial, (int)blocks, n, G, KP, c.m.p, S,
				   brow, ctl);
}

/* word width, reducer and KP once, then one of the two launches */
template <typename W, int MERS>
static hipError_t border_k_kp(const KernelCfg &c, bool update, void *T, const void *B, void *S, const long long *brow, int k,
			      long long rows, u64 *partial, u64 *send, const DevCtl *ctl, hipStream_t s)
{
	const bool known = with_lane_group<2, 4, 8, 16>(border_kp(k), [&](auto kt) {
		constexpr int KP = decltype(kt)::value;
		if (update)
			border_update_k_go<W, MERS, KP>(c, (W *)T, (const W *)B, (const W *)S, brow, k, rows, ctl, s);
		else
			border_dot_k_go<W, MERS, KP>(c, (const W *)T, (const W *)B, rows, partial, (W *)S, brow, k, send, ctl, s);
	});
	return known ? hipGetLastError() : hipErrorInvalidValue;
}

static hipError_t border_k(const KernelCfg &c, bool update, void *T, const void *B, void *S, const long long *brow, int k,
			   int64_t rows, u64 *partial, u64 *send, const DevCtl *ctl, hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN || k < 2 || k > BLZ_BORDER_MAXK)
		return hipErrorInvalidValue;
	if (update && rows <= 0)
		return hipSuccess;
	return with_word_reducer(c, [&](auto wt, auto mers) {
		return border_k_kp<typename decltype(wt)::type, decltype(mers)::value>(c, update, T, B, S, brow, k, rows, partial, send, ctl, s);
	});
}

hipError_t launch_border_update_k(const KernelCfg &c, void *T, const void *B, const void *V, const long long *brow, int k,
				  int64_t rows, const DevCtl *ctl, hipStream_t s)
{
	return border_k(c, true, T, B, const_cast<void *>(V), brow, k, rows, nullptr, nullptr, ctl, s);
}

hipError_t launch_border_dot_k(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, void *S,
			       const long long *brow, int k, const DevCtl *ctl, hipStream_t s)
{
	return border_k(c, false, const_cast<void *>(T), B, S, brow, k, rows, partial, nullptr, ctl, s);
}

/* ---- several ranks: the rank's share of the dot into a send buffer, the all-reduced rows into the slab ---- */

hipError_t launch_border_dot_send(const KernelCfg &c, const void *T, const void *B, int64_t rows, u64 *partial, u64 *send, int k,
				  const DevCtl *ctl, hipStream_t s)
{
	if (!send)
		return hipErrorInvalidValue;
	if (k == 1)
		return border_dot_go(c, T, B, rows, partial, nullptr, send, ctl, s);
	return border_k(c, false, const_cast<void *>(T), B, nullptr, nullptr, k, rows, partial, send, ctl, s);
}

hipError_t launch_border_place(const KernelCfg &c, const u64 *recv, void *S, const long long *own, int k, const DevCtl *ctl,
			       hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN || k < 1 || k > BLZ_BORDER_MAXK)
		return hipErrorInvalidValue;
	const dim3 grid(1), blk(BLOCK);
	if (c.word == 4)	/* (the sums of 32-bit residues go through Barrett at either reducer class, as in k_reduce_modp) */
		hipLaunchKernelGGL((k_border_place<u32, 0>), grid, blk, 0, s, recv, k, c.n, c.m, (u32 *)S, own, ctl);
	else if (c.mers == 61)
		hipLaunchKernelGGL((k_border_place<u64, 61>), grid, blk, 0, s, recv, k, c.n, c.m, (u64 *)S, own, ctl);
	else
		hipLaunchKernelGGL((k_border_place<u64, 0>), grid, blk, 0, s, recv, k, c.n, c.m, (u64 *)S, own, ctl);
	return hipGetLastError();
}

hipError_t launch_border_rows_send(const KernelCfg &c, const void *V, const long long *own, int k, u64 *send, hipStream_t s)
{
	if (c.n < 1 || c.n > BLZ_BORDER_MAXN || k < 1 || k > BLZ_BORDER_MAXK)
		return hipErrorInvalidValue;
	if (c.word == 4)
		hipLaunchKernelGGL((k_border_rows_send<u32>), dim3(1), dim3(BLOCK), 0, s, (const u32 *)V, own, k, c.n, send);
	else
		hipLaunchKernelGGL((k_border_rows_send<u64>), dim3(1), dim3(BLOCK), 0, s, (const u64 *)V, own, k, c.n, send);
	return hipGetLastError();
}
