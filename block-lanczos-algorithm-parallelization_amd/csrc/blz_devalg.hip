/*
 * blz_devalg.hip -- device block algebra: the two dense parts of a Krylov step on a caller's blocks in device memory,
 *     k_dev_dot       C = X^T * Y mod p          (n x n out of two tall rows x n blocks)
 *     k_dev_combine   Z = sum_t X_t * A_t mod p  (row-local, up to four terms, in place allowed)
 * A block is rows x n u64 words with a row stride of ld >= n words; the words n .. ld-1 of a row are never touched.  Both
 * operations are invariant under a permutation of the rows, so unlike blz_apply_device nothing is imported into a slab: the
 * kernels stream the caller's rows where they lie.  Sums of 64 x 64 -> 128-bit products are kept unreduced for at most
 * ModP::chunk products (modp.h: 1 at p = 2^62 - 57, 32 at 2^61 - 1; the 96-bit AccS of p < 2^32 takes 2^32 of them and is
 * reduced every 2^31), and every word written is the canonical residue of the exact integer sum.
 *
 * k_dev_dot.  Tiles of TR = 1024 >> lg consecutive rows (lg = log2 of the next power of two >= n: 128 rows at n = 8, 16 at
 * n = 64) go round-robin over the workgroups.  A tile of X and one of Y are staged through LDS (8 KB each; one of them when
 * X is Y), loaded by lane groups of one row each -- contiguous 8-byte or, where pointer, stride and width allow, 16-byte lane
 * accesses -- and the loads of the next tile are issued into registers before the current one is multiplied.  An LDS row is
 * padded with zeros to the power of two.  For n > 16 a thread owns the entries e = t, t + 256, ... of C (i = e / n from X,
 * j = e % n from Y: adjacent lanes read adjacent words of Y's row and broadcast X's).  For n <= 16 a thread owns a 2 x 2
 * tile of C (two 16-byte LDS reads per four products, four independent sums) and, n * n / 4 being less than 256, the threads
 * also split the tile's rows into slices that are added in LDS at the end.  Each workgroup writes ONE row of n * n residues
 * to the context's scratch and k_dev_dot_finalize adds the rows mod p: no atomics, no host round trip.
 *
 * k_dev_combine.  The coefficient matrices sit in LDS (nterms * n * n words: 128 KB for four terms at n = 64, then one
 * workgroup of 1024 threads per CU; 256 threads otherwise).  A lane group of G lanes takes one row: every lane loads its
 * word (or pair of words) of the row of EVERY term into registers, the words reach the other lanes by shuffles, and only
 * then is the row of Z stored -- which is what makes Z = one of the X_t safe.
 */
#include "blz_devalg.h"

#include <type_traits>

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_WORDS = 1024;	/* one block's tile: (TILE_WORDS >> lg) rows of at most (1 << lg) words */

__device__ __forceinline__ u64 shfl64(u64 v, int src)
{
	return (u64)__shfl((unsigned long long)v, src, 64);
}

/* the words of a tile a thread moves: K = 4 rows of one word, or 2 rows of two words */
template <bool VEC2>
struct TileRegs {
	u64 w[4];
};

/* rows [row0, row0 + TR) of a block into registers; a lane group of (1 << lgu) lanes per row, `units` of them live */
template <bool VEC2>
__device__ __forceinline__ void tile_load(TileRegs<VEC2> &g, const u64 *__restrict__ b, long long ld, long long row0, long long rows,
					  int units, int lgu)
{
	const int lane = threadIdx.x & ((1 << lgu) - 1), rsub = threadIdx.x >> lgu, rpp = BLOCK >> lgu;
#pragma unroll
	for (int k = 0; k < (VEC2 ? 2 : 4); k++) {
		const long long row = row0 + rsub + k * rpp;
		const bool live = lane < units && row < rows;
		if constexpr (VEC2) {
			ulonglong2 v = make_ulonglong2(0, 0);
			if (live)
				v = *reinterpret_cast<const ulonglong2 *>(b + row * ld + 2 * lane);
			g.w[2 * k] = v.x;
			g.w[2 * k + 1] = v.y;
		} else {
			g.w[k] = live ? b[row * ld + lane] : 0;
		}
	}
}

/* the same words into the LDS tile, (1 << lg) words per row: the columns past n and the rows past the block's end arrive
 * as zeros (the lanes of a row cover the whole pitch, a dead lane's registers are zero) */
template <bool VEC2>
__device__ __forceinline__ void tile_store(const TileRegs<VEC2> &g, u64 *tile, int pitch, int lgu)
{
	const int lane = threadIdx.x & ((1 << lgu) - 1), rsub = threadIdx.x >> lgu, rpp = BLOCK >> lgu;
#pragma unroll
	for (int k = 0; k < (VEC2 ? 2 : 4); k++) {
		const int r = rsub + k * rpp;
		if constexpr (VEC2)
			*reinterpret_cast<ulonglong2 *>(tile + r * pitch + 2 * lane) = make_ulonglong2(g.w[2 * k], g.w[2 * k + 1]);
		else
			tile[r * pitch + lane] = g.w[k];
	}
}

/* NP = entries of C per thread for n > 16: 4 (n <= 32) or 16 (n <= 64), entries t, t + 256, ...
 * NP == 1 is n <= 16: a thread owns a TT x TT tile of C (TT = 2; 1 at n = 1) -- two 16-byte LDS reads per four products and
 * four independent sums -- and the 256 / (pitch / TT)^2 slices of threads split the tile's rows. */
template <bool NARROW, int MERS, int NP, int TT, bool VEC2>
__global__ void __launch_bounds__(BLOCK)
k_dev_dot(const u64 *__restrict__ x, long long ldx, const u64 *__restrict__ y, long long ldy, long long rows, int n, int lg,
	  ModP m, u64 *__restrict__ partial)
{
	using A = typename std::conditional<NARROW, AccS, typename std::conditional<(NP <= 4), AccL, Acc>::type>::type;
	constexpr int NACC = NP == 1 ? TT * TT : NP;
	__shared__ __attribute__((aligned(16))) u64 xs[TILE_WORDS];
	__shared__ __attribute__((aligned(16))) u64 ys[TILE_WORDS];
	const bool gram = x == y && ldx == ldy;
	const u64 *yt = gram ? xs : ys;
	const int t = threadIdx.x, pairs = n * n, pitch = 1 << lg, TR = TILE_WORDS >> lg;
	const int units = VEC2 ? n >> 1 : n, lgu = VEC2 ? lg - 1 : lg;
	const int tpr = pitch / TT, tps = tpr * tpr;	/* NP == 1: tiles per row and column of C, threads per slice */
	const int slices = NP == 1 ? BLOCK / tps : 1, slice = NP == 1 ? t / tps : 0;
	const u32 chunk = NARROW ? 0x80000000u : m.chunk;
	A acc[NACC];
	int xi[NP], yj[NP];
#pragma unroll
	for (int q = 0; q < NACC; q++)
		acc_zero(acc[q]);
#pragma unroll
	for (int q = 0; q < NP; q++) {
		if (NP == 1) {
			xi[q] = TT * ((t % tps) / tpr);	/* first row and column of the thread's tile */
			yj[q] = TT * ((t % tps) % tpr);
		} else {
			const int e = t + q * BLOCK;
			xi[q] = e < pairs ? e / n : 0;	/* (an entry past the end multiplies words 0 and is not written) */
			yj[q] = e < pairs ? e % n : 0;
		}
	}
	u32 cnt = 0;
	const long long ntiles = (rows + TR - 1) / TR;
	long long tile = blockIdx.x;
	TileRegs<VEC2> gx, gy;
	if (tile < ntiles) {
		tile_load<VEC2>(gx, x, ldx, tile * TR, rows, units, lgu);
		if (!gram)
			tile_load<VEC2>(gy, y, ldy, tile * TR, rows, units, lgu);
	}
	while (tile < ntiles) {
		__syncthreads();	/* the tile before this one has been read */
		tile_store<VEC2>(gx, xs, pitch, lgu);
		if (!gram)
			tile_store<VEC2>(gy, ys, pitch, lgu);
		__syncthreads();
		const long long next = tile + gridDim.x;
		if (next < ntiles) {	/* in flight while this tile is multiplied */
			tile_load<VEC2>(gx, x, ldx, next * TR, rows, units, lgu);
			if (!gram)
				tile_load<VEC2>(gy, y, ldy, next * TR, rows, units, lgu);
		}
		const long long left = rows - tile * TR;
		const int tr = left < TR ? (int)left : TR;
		for (int r = slice; r < tr; r += slices) {
			const u64 *xr = xs + r * pitch, *yr = yt + r * pitch;
			if constexpr (NP == 1 && TT == 2) {
				const ulonglong2 xa = *reinterpret_cast<const ulonglong2 *>(xr + xi[0]);
				const ulonglong2 ya = *reinterpret_cast<const ulonglong2 *>(yr + yj[0]);
				acc_mac64(acc[0], xa.x, ya.x);
				acc_mac64(acc[1], xa.x, ya.y);
				acc_mac64(acc[2], xa.y, ya.x);
				acc_mac64(acc[3], xa.y, ya.y);
			} else {
#pragma unroll
				for (int q = 0; q < NP; q++)
					acc_mac64(acc[q], xr[xi[q]], yr[yj[q]]);
			}
			if (++cnt == chunk) {
				cnt = 0;
#pragma unroll
				for (int q = 0; q < NACC; q++)
					acc_set(acc[q], acc_reduce<MERS>(acc[q], m));
			}
		}
		tile = next;
	}
	u64 *out = partial + (size_t)blockIdx.x * pairs;
	if constexpr (NP == 1) {
		__syncthreads();	/* xs is free: the slices' residues, [entry of the tile][thread] -- NACC * 256 <= 1024 words */
#pragma unroll
		for (int q = 0; q < NACC; q++)
			xs[q * BLOCK + t] = acc_reduce<MERS>(acc[q], m);
		__syncthreads();
		if (t < pairs) {
			const int i = t / n, j = t % n;
			const u64 *mine = xs + ((i % TT) * TT + (j % TT)) * BLOCK + (i / TT) * tpr + (j / TT);
			u64 s = 0;
			for (int sl = 0; sl < slices; sl++)
				s = addmod(s, mine[sl * tps], m.p);
			out[t] = s;
		}
	} else {
#pragma unroll
		for (int q = 0; q < NP; q++) {
			const int e = t + q * BLOCK;
			if (e < pairs)
				out[e] = acc_reduce<MERS>(acc[q], m);
		}
	}
}

/* out[e] = sum_b partial[b][e] mod p, e < words.  A workgroup owns 8 adjacent words, a thread is (row lane, word): a
 * wavefront's load covers 8 partial rows x 64 bytes.  nblocks == 0: zeros. */
__global__ void __launch_bounds__(BLOCK)
k_dev_dot_finalize(const u64 *__restrict__ partial, int nblocks, int words, u64 p, u64 *__restrict__ out)
{
	__shared__ u64 red[BLOCK];
	const int wl = threadIdx.x & 7, rl = threadIdx.x >> 3, e = blockIdx.x * 8 + wl;
	u64 s = 0;
	if (e < words)
		for (int b = rl; b < nblocks; b += BLOCK / 8)
			s = addmod(s, partial[(size_t)b * words + e], p);
	red[threadIdx.x] = s;
	__syncthreads();
	if (threadIdx.x < 8 && e < words) {
		u64 tsum = 0;
		for (int r = 0; r < BLOCK / 8; r++)
			tsum = addmod(tsum, red[r * 8 + threadIdx.x], p);
		out[e] = tsum;
	}
}

struct CombineArgs {
	const u64 *x[DEVALG_MAX_TERMS];
	long long ldx[DEVALG_MAX_TERMS];
	const u64 *a[DEVALG_MAX_TERMS];
};

/* a lane group of (1 << lg) lanes per row; a lane owns column `col` (VEC2: columns 2 col and 2 col + 1) */
template <bool NARROW, int MERS, bool VEC2>
__global__ void __launch_bounds__(1024)
k_dev_combine(CombineArgs g, int nterms, u64 *z, long long ldz, long long rows, int n, int lg, ModP m)
{
	using A = typename std::conditional<NARROW, AccS, AccL>::type;
	extern __shared__ __attribute__((aligned(16))) u64 As[];	/* [term][i * n + j] */
	const int nn = n * n;
	for (int t = 0; t < nterms; t++)
		for (int k = threadIdx.x; k < nn; k += blockDim.x)
			As[t * nn + k] = g.a[t][k];
	__syncthreads();
	const int G = 1 << lg, lane = threadIdx.x & 63, col = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg;
	const int units = VEC2 ? n >> 1 : n, wpb = blockDim.x >> 6;
	const int cj = col < units ? col : 0;	/* an idle lane multiplies column 0 and stores nothing */
	const u32 chunk = NARROW ? 0x80000000u : m.chunk;
	const long long groups = (rows + rpw - 1) / rpw;
	for (long long grp = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); grp < groups; grp += (long long)gridDim.x * wpb) {
		const long long row = grp * rpw + sub;
		const bool mine = row < rows && col < units;
		u64 xv[DEVALG_MAX_TERMS][VEC2 ? 2 : 1];
#pragma unroll
		for (int t = 0; t < DEVALG_MAX_TERMS; t++) {	/* the whole row of every term, before anything is stored */
			const bool ld_ = mine && t < nterms;
			if constexpr (VEC2) {
				ulonglong2 v = make_ulonglong2(0, 0);
				if (ld_)
					v = *reinterpret_cast<const ulonglong2 *>(g.x[t] + row * g.ldx[t] + 2 * col);
				xv[t][0] = v.x;
				xv[t][1] = v.y;
			} else {
				xv[t][0] = ld_ ? g.x[t][row * g.ldx[t] + col] : 0;
			}
		}
		A acc[VEC2 ? 2 : 1];
		acc_zero(acc[0]);
		if constexpr (VEC2)
			acc_zero(acc[1]);
		u32 cnt = 0;
#pragma unroll
		for (int t = 0; t < DEVALG_MAX_TERMS; t++) {
			if (t >= nterms)
				break;
			const u64 *At = As + t * nn;
			if constexpr (VEC2) {
				for (int i = 0; i < n; i += 2) {
					const u64 x0 = shfl64(xv[t][0], sub * G + (i >> 1)), x1 = shfl64(xv[t][1], sub * G + (i >> 1));
#pragma unroll
					for (int h = 0; h < 2; h++) {
						const ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(At + (i + h) * n + 2 * cj);
						acc_mac64(acc[0], h ? x1 : x0, av.x);
						acc_mac64(acc[1], h ? x1 : x0, av.y);
						if (++cnt == chunk) {
							cnt = 0;
							acc_set(acc[0], acc_reduce<MERS>(acc[0], m));
							acc_set(acc[1], acc_reduce<MERS>(acc[1], m));
						}
					}
				}
			} else {
				for (int i = 0; i < n; i++) {
					acc_mac64(acc[0], shfl64(xv[t][0], sub * G + i), At[i * n + cj]);
					if (++cnt == chunk) {
						cnt = 0;
						acc_set(acc[0], acc_reduce<MERS>(acc[0], m));
					}
				}
			}
		}
		if (mine) {
			if constexpr (VEC2)
				*reinterpret_cast<ulonglong2 *>(z + row * ldz + 2 * col) =
					make_ulonglong2(acc_reduce<MERS>(acc[0], m), acc_reduce<MERS>(acc[1], m));
			else
				z[row * ldz + col] = acc_reduce<MERS>(acc[0], m);
		}
	}
}

inline int log2_ceil(int v)
{
	int lg = 0;
	while ((1 << lg) < v)
		lg++;
	return lg;
}

/* 16-byte lane accesses: an even width, an even stride and a 16-byte aligned base */
inline bool pair_ok(const void *b, long long ld, int n)
{
	return (n & 1) == 0 && (ld & 1) == 0 && ((uintptr_t)b & 15) == 0;
}

template <bool NARROW, int MERS, int NP, int TT>
void dot_go(bool v2, unsigned grid, hipStream_t s, const u64 *x, long long ldx, const u64 *y, long long ldy, long long rows, int n,
	    int lg, const ModP &m, u64 *partial)
{
	if (v2)
		hipLaunchKernelGGL((k_dev_dot<NARROW, MERS, NP, TT, true>), dim3(grid), dim3(BLOCK), 0, s, x, ldx, y, ldy, rows, n, lg, m, partial);
	else
		hipLaunchKernelGGL((k_dev_dot<NARROW, MERS, NP, TT, false>), dim3(grid), dim3(BLOCK), 0, s, x, ldx, y, ldy, rows, n, lg, m, partial);
}

template <bool NARROW, int MERS>
void dot_np(int np, bool v2, unsigned grid, hipStream_t s, const u64 *x, long long ldx, const u64 *y, long long ldy, long long rows,
	    int n, int lg, const ModP &m, u64 *partial)
{
	if (np == 1 && n == 1)
		dot_go<NARROW, MERS, 1, 1>(v2, grid, s, x, ldx, y, ldy, rows, n, lg, m, partial);
	else if (np == 1)
		dot_go<NARROW, MERS, 1, 2>(v2, grid, s, x, ldx, y, ldy, rows, n, lg, m, partial);
	else if (np == 4)
		dot_go<NARROW, MERS, 4, 1>(v2, grid, s, x, ldx, y, ldy, rows, n, lg, m, partial);
	else
		dot_go<NARROW, MERS, 16, 1>(v2, grid, s, x, ldx, y, ldy, rows, n, lg, m, partial);
}

template <bool NARROW, int MERS, bool VEC2>
void combine_go(unsigned grid, unsigned block, size_t lds, hipStream_t s, const CombineArgs &g, int nterms, u64 *z, long long ldz,
		long long rows, int n, int lg, const ModP &m)
{
	if (lds > 48 * 1024)
		(void)hipFuncSetAttribute((const void *)k_dev_combine<NARROW, MERS, VEC2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	hipLaunchKernelGGL((k_dev_combine<NARROW, MERS, VEC2>), dim3(grid), dim3(block), lds, s, g, nterms, z, ldz, rows, n, lg, m);
}

template <bool NARROW, int MERS>
void combine_v(bool v2, unsigned grid, unsigned block, size_t lds, hipStream_t s, const CombineArgs &g, int nterms, u64 *z,
	       long long ldz, long long rows, int n, int lg, const ModP &m)
{
	if (v2)
		combine_go<NARROW, MERS, true>(grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, m);
	else
		combine_go<NARROW, MERS, false>(grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, m);
}

}  // namespace

/* the scratch stays at 8 MB at n = 64 (256 partial rows of 32 KB) and below it elsewhere */
int dev_dot_max_blocks(const KernelCfg &c, int n)
{
	const long long by_bytes = ((long long)8 << 20) / ((long long)n * n * 8), by_cu = (long long)c.num_cu * 4;
	const long long b = by_bytes < by_cu ? by_bytes : by_cu;
	return (int)(b < 1 ? 1 : b);
}

hipError_t launch_dev_dot(const KernelCfg &c, int n, long long rows, const u64 *x, long long ldx, const u64 *y, long long ldy,
			  u64 *partial, u64 *out, hipStream_t s)
{
	if (n < 1 || n > 64 || rows < 0)
		return hipErrorInvalidValue;
	const int lg = log2_ceil(n), TR = TILE_WORDS >> lg, words = n * n;
	const long long ntiles = (rows + TR - 1) / TR, cap = dev_dot_max_blocks(c, n);
	const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
	if (grid) {
		const int np = words <= BLOCK ? 1 : words <= 4 * BLOCK ? 4 : 16;
		const bool v2 = pair_ok(x, ldx, n) && pair_ok(y, ldy, n);
		const bool narrow = c.m.p < (1ull << 32);
		if (narrow && c.mers == 31)
			dot_np<true, 31>(np, v2, grid, s, x, ldx, y, ldy, rows, n, lg, c.m, partial);
		else if (narrow)
			dot_np<true, 0>(np, v2, grid, s, x, ldx, y, ldy, rows, n, lg, c.m, partial);
		else if (c.mers == 61)
			dot_np<false, 61>(np, v2, grid, s, x, ldx, y, ldy, rows, n, lg, c.m, partial);
		else
			dot_np<false, 0>(np, v2, grid, s, x, ldx, y, ldy, rows, n, lg, c.m, partial);
	}
	hipLaunchKernelGGL(k_dev_dot_finalize, dim3((unsigned)((words + 7) / 8)), dim3(BLOCK), 0, s, partial, (int)grid, words, c.m.p, out);
	return hipGetLastError();
}

hipError_t launch_dev_combine(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			      const u64 *const *a, u64 *z, long long ldz, hipStream_t s)
{
	if (n < 1 || n > 64 || nterms < 1 || nterms > DEVALG_MAX_TERMS || rows < 0)
		return hipErrorInvalidValue;
	if (rows == 0)
		return hipSuccess;
	CombineArgs g{};
	bool v2 = pair_ok(z, ldz, n);
	for (int t = 0; t < nterms; t++) {
		g.x[t] = x[t];
		g.ldx[t] = ldx[t];
		g.a[t] = a[t];
		v2 = v2 && pair_ok(x[t], ldx[t], n);
	}
	const int lg = log2_ceil(v2 ? n / 2 : n), rpw = 64 >> lg;
	const size_t lds = (size_t)nterms * n * n * sizeof(u64);
	const unsigned block = lds > 40 * 1024 ? 1024 : BLOCK;	/* a workgroup per CU then: make it a full one */
	const long long wpb = block / 64, groups = (rows + rpw - 1) / rpw, want = (groups + wpb - 1) / wpb;
	const long long cap = (long long)c.num_cu * (block == 1024 ? 1 : 8);
	const unsigned grid = (unsigned)(want < cap ? want : cap);
	const bool narrow = c.m.p < (1ull << 32);
	if (narrow && c.mers == 31)
		combine_v<true, 31>(v2, grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, c.m);
	else if (narrow)
		combine_v<true, 0>(v2, grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, c.m);
	else if (c.mers == 61)
		combine_v<false, 61>(v2, grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, c.m);
	else
		combine_v<false, 0>(v2, grid, block, lds, s, g, nterms, z, ldz, rows, n, lg, c.m);
	return hipGetLastError();
}
