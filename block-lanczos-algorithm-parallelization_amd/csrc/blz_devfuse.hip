/*
 * blz_devfuse.hip -- fused device block algebra: the two dense parts of a Krylov step, each in ONE pass over the caller's blocks,
 *     k_dev_dot2       C0 = X0^T * Y, C1 = X1^T * Y mod p                    (two n x n panels out of up to three tall blocks)
 *     k_dev_combine2   Z0 = sum_t X_t * A0_t, Z1 = sum_t X_t * A1_t mod p     (row-local, up to four terms, in place allowed)
 * The conventions are those of blz_devalg.hip: a block is rows x n u64 words with a row stride of ld >= n words, the words
 * n .. ld-1 of a row are never touched, sums of 64 x 64 -> 128-bit products are kept unreduced for at most ModP::chunk
 * products per accumulator, and every word written is the canonical residue of the exact integer sum.  The small helpers of
 * that file (the tile loads and stores, the shuffle, log2_ceil, pair_ok, the finalize) are restated here: that file and its
 * kernels stay as they are.
 *
 * k_dev_dot2 has the tile loop of k_dev_dot.  Blocks that are the same pointer with the same stride are ONE block: the
 * launcher passes the distinct blocks (one to three) and which of them X0, X1 and Y are, and a tile of 1024 words of each
 * distinct block is staged through LDS (24 KB at the most), the loads of the next tile in registers while this one is
 * multiplied.  A thread owns the same entries of both panels -- entries t, t + 256, ... at n > 16, a 2 x 2 tile and a slice of
 * the tile's rows at n <= 16 -- so the word of Y it reads is multiplied into two accumulators.  A workgroup writes one row of
 * 2 * n * n residues ([panel][entry]) to the call's own scratch and k_dev_dot2_finalize adds the rows mod p.  At n > 32 a thread
 * holds two sets of 16 accumulators: the 96-bit ones of p < 2^32 and the 128-bit ones of p = 2^61 - 1 fit the 256 registers of
 * a lane, those of the Barrett class (one set alone takes 244) do not without moving a set to the accumulation registers, so
 * that class runs launch_dev_dot twice inside the one call at those widths (dot has no in-place form: that is correct).
 *
 * k_dev_combine2 has the lane-group loop of k_dev_combine.  The coefficient panels of a term sit in LDS when they fit --
 * 160 KB hold five panels at n = 64, as one workgroup of 1024 threads with nothing else in LDS -- and the terms whose panels
 * do not fit read theirs from global memory, through the cache (32 KB each at the most, the same for every workgroup).  It is
 * ONE launch at every panel count: a lane group holds its row of every term in registers before it stores either output row,
 * which is what makes each of Z0 and Z1 = one of the X_t safe, and what a second launch would break.
 */
#include "blz_devfuse.h"

#include <type_traits>

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_WORDS = 1024;	/* one block's tile: (TILE_WORDS >> lg) rows of at most (1 << lg) words */
constexpr int DOT2_BLOCKS = 3;		/* X0, X1 and Y, when all are distinct */
constexpr int DOT2_BARRETT_MAX_N = 32;	/* beyond: two sets of 16 Acc per thread, see above */
constexpr size_t LDS_BYTES = 160 * 1024;	/* of a CU, all of which one workgroup may have */

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

/* the same words into the LDS tile, (1 << lg) words per row: the columns past n and the rows past the block's end arrive as
 * zeros (the lanes of a row cover the whole pitch, a dead lane's registers are zero) */
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

/* the distinct blocks of a call, and which of them X0, X1 and Y are */
struct Dot2Args {
	const u64 *b[DOT2_BLOCKS];
	long long ld[DOT2_BLOCKS];
	int nblk, ix0, ix1, iy;
};

/* NP, TT: as in k_dev_dot (NP = 16 at n > 32, 4 at 16 < n <= 32; NP == 1 is n <= 16, a TT x TT tile per thread and slices of rows).
 * acc[0] belongs to C0 = X0^T Y, acc[1] to C1 = X1^T Y; both take one product per row, so one count serves the chunk rule. */
template <bool NARROW, int MERS, int NP, int TT, bool VEC2>
__global__ void __launch_bounds__(BLOCK)
k_dev_dot2(Dot2Args g, long long rows, int n, int lg, ModP m, u64 *__restrict__ partial)
{
	using A = typename std::conditional<NARROW, AccS, typename std::conditional<(NP <= 4), AccL, Acc>::type>::type;
	constexpr int NACC = NP == 1 ? TT * TT : NP;
	__shared__ __attribute__((aligned(16))) u64 tiles[DOT2_BLOCKS * TILE_WORDS];
	const u64 *x0t = tiles + g.ix0 * TILE_WORDS, *x1t = tiles + g.ix1 * TILE_WORDS, *yt = tiles + g.iy * TILE_WORDS;
	const int t = threadIdx.x, pairs = n * n, pitch = 1 << lg, TR = TILE_WORDS >> lg;
	const int units = VEC2 ? n >> 1 : n, lgu = VEC2 ? lg - 1 : lg;
	const int tpr = pitch / TT, tps = tpr * tpr;	/* NP == 1: tiles per row and column of a panel, threads per slice */
	const int slices = NP == 1 ? BLOCK / tps : 1, slice = NP == 1 ? t / tps : 0;
	const u32 chunk = NARROW ? 0x80000000u : m.chunk;
	A acc[2][NACC];
	int xi[NP], yj[NP];
#pragma unroll
	for (int q = 0; q < NACC; q++) {
		acc_zero(acc[0][q]);
		acc_zero(acc[1][q]);
	}
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
	TileRegs<VEC2> gr[DOT2_BLOCKS];
	if (tile < ntiles) {
#pragma unroll
		for (int k = 0; k < DOT2_BLOCKS; k++)
			if (k < g.nblk)
				tile_load<VEC2>(gr[k], g.b[k], g.ld[k], tile * TR, rows, units, lgu);
	}
	while (tile < ntiles) {
		__syncthreads();	/* the tile before this one has been read */
#pragma unroll
		for (int k = 0; k < DOT2_BLOCKS; k++)
			if (k < g.nblk)
				tile_store<VEC2>(gr[k], tiles + k * TILE_WORDS, pitch, lgu);
		__syncthreads();
		const long long next = tile + gridDim.x;
		if (next < ntiles) {	/* in flight while this tile is multiplied */
#pragma unroll
			for (int k = 0; k < DOT2_BLOCKS; k++)
				if (k < g.nblk)
					tile_load<VEC2>(gr[k], g.b[k], g.ld[k], next * TR, rows, units, lgu);
		}
		const long long left = rows - tile * TR;
		const int tr = left < TR ? (int)left : TR;
		for (int r = slice; r < tr; r += slices) {
			const u64 *x0r = x0t + r * pitch, *x1r = x1t + r * pitch, *yr = yt + r * pitch;
			if constexpr (NP == 1 && TT == 2) {
				const ulonglong2 xa = *reinterpret_cast<const ulonglong2 *>(x0r + xi[0]);
				const ulonglong2 xb = *reinterpret_cast<const ulonglong2 *>(x1r + xi[0]);
				const ulonglong2 ya = *reinterpret_cast<const ulonglong2 *>(yr + yj[0]);
				acc_mac64(acc[0][0], xa.x, ya.x);
				acc_mac64(acc[0][1], xa.x, ya.y);
				acc_mac64(acc[0][2], xa.y, ya.x);
				acc_mac64(acc[0][3], xa.y, ya.y);
				acc_mac64(acc[1][0], xb.x, ya.x);
				acc_mac64(acc[1][1], xb.x, ya.y);
				acc_mac64(acc[1][2], xb.y, ya.x);
				acc_mac64(acc[1][3], xb.y, ya.y);
			} else {
#pragma unroll
				for (int q = 0; q < NP; q++) {
					const u64 yv = yr[yj[q]];
					acc_mac64(acc[0][q], x0r[xi[q]], yv);
					acc_mac64(acc[1][q], x1r[xi[q]], yv);
				}
			}
			if (++cnt == chunk) {
				cnt = 0;
#pragma unroll
				for (int q = 0; q < NACC; q++) {
					acc_set(acc[0][q], acc_reduce<MERS>(acc[0][q], m));
					acc_set(acc[1][q], acc_reduce<MERS>(acc[1][q], m));
				}
			}
		}
		tile = next;
	}
	u64 *out = partial + (size_t)blockIdx.x * 2 * pairs;
	if constexpr (NP == 1) {
		__syncthreads();	/* the tiles are free: the slices' residues, [panel][entry of the tile][thread] -- NACC * 256 <= 1024 words a panel */
#pragma unroll
		for (int s = 0; s < 2; s++)
#pragma unroll
			for (int q = 0; q < NACC; q++)
				tiles[s * TILE_WORDS + q * BLOCK + t] = acc_reduce<MERS>(acc[s][q], m);
		__syncthreads();
		if (t < pairs) {
			const int i = t / n, j = t % n;
#pragma unroll
			for (int s = 0; s < 2; s++) {
				const u64 *mine = tiles + s * TILE_WORDS + ((i % TT) * TT + (j % TT)) * BLOCK + (i / TT) * tpr + (j / TT);
				u64 sum = 0;
				for (int sl = 0; sl < slices; sl++)
					sum = addmod(sum, mine[sl * tps], m.p);
				out[s * pairs + t] = sum;
			}
		}
	} else {
#pragma unroll
		for (int q = 0; q < NP; q++) {
			const int e = t + q * BLOCK;
			if (e < pairs) {
				out[e] = acc_reduce<MERS>(acc[0][q], m);
				out[pairs + e] = acc_reduce<MERS>(acc[1][q], m);
			}
		}
	}
}

/* out[e] = sum_b partial[b][e] mod p, e < words (= 2 * n * n).  A workgroup owns 8 adjacent words, a thread is (row lane,
 * word): a wavefront's load covers 8 partial rows x 64 bytes.  nblocks == 0: zeros. */
__global__ void __launch_bounds__(BLOCK)
k_dev_dot2_finalize(const u64 *__restrict__ partial, int nblocks, int words, u64 p, u64 *__restrict__ out)
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

/* entry t of four, by selects: a register array indexed by a loop counter would live in scratch */
template <class T>
__device__ __forceinline__ T pick4(int t, T v0, T v1, T v2, T v3)
{
	return t == 0 ? v0 : t == 1 ? v1 : t == 2 ? v2 : v3;
}

/* a[o][t]: the panel of term t in output o or NULL; where[t]: the place in LDS, in panels, of the term's first present
 * panel (the second, when both are present, follows it), or -1: the term reads its panels from global memory */
struct Combine2Args {
	const u64 *x[DEVALG_MAX_TERMS];
	long long ldx[DEVALG_MAX_TERMS];
	const u64 *a[2][DEVALG_MAX_TERMS];
	int where[DEVALG_MAX_TERMS];
};

/* what one word of a term's row needs: the word itself, from the lane that holds it, and the words of row i of the term's
 * panels under this lane's column(s).  A panel in global memory (GLB) is aligned to 8 bytes only: no 16-byte loads there. */
template <bool VEC2>
struct Combine2Step {
	u64 xw, a0[VEC2 ? 2 : 1], a1[VEC2 ? 2 : 1];
};

template <bool VEC2, bool H0, bool H1, bool GLB>
__device__ __forceinline__ void combine2_fetch(Combine2Step<VEC2> &f, int i, u64 xlo, u64 xhi, const u64 *A0, const u64 *A1, int n,
					       int G, int sub, int cj)
{
	if constexpr (VEC2) {	/* word i of the row: the low or the high word of lane i / 2 */
		f.xw = shfl64((i & 1) ? xhi : xlo, sub * G + (i >> 1));
		const int at = i * n + 2 * cj;
		if constexpr (H0) {
			if constexpr (GLB) {
				f.a0[0] = A0[at];
				f.a0[1] = A0[at + 1];
			} else {
				const ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(A0 + at);
				f.a0[0] = av.x;
				f.a0[1] = av.y;
			}
		}
		if constexpr (H1) {
			if constexpr (GLB) {
				f.a1[0] = A1[at];
				f.a1[1] = A1[at + 1];
			} else {
				const ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(A1 + at);
				f.a1[0] = av.x;
				f.a1[1] = av.y;
			}
		}
	} else {
		f.xw = shfl64(xlo, sub * G + i);
		if constexpr (H0)
			f.a0[0] = A0[i * n + cj];
		if constexpr (H1)
			f.a1[0] = A1[i * n + cj];
	}
}

template <bool VEC2, bool H0, bool H1, class A>
__device__ __forceinline__ void combine2_mac(A (&acc)[2][VEC2 ? 2 : 1], const Combine2Step<VEC2> &f)
{
#pragma unroll
	for (int k = 0; k < (VEC2 ? 2 : 1); k++) {
		if constexpr (H0)
			acc_mac64(acc[0][k], f.xw, f.a0[k]);
		if constexpr (H1)
			acc_mac64(acc[1][k], f.xw, f.a1[k]);
	}
}

/* one term into the accumulators of the outputs it enters (H0, H1); A0 and A1 are its panels, in LDS or (GLB) in global
 * memory.  The n words of the row go in runs of at most chunk - cnt, the room the accumulators have left, with the reduction
 * BETWEEN runs: the loop that multiplies has no branch in it and takes two words a turn, so the shuffle and the panel words
 * of the second are on their way while the first is multiplied. */
template <int MERS, bool VEC2, bool H0, bool H1, bool GLB, class A>
__device__ __forceinline__ void combine2_term(A (&acc)[2][VEC2 ? 2 : 1], u32 &cnt, u32 chunk, const u64 (&xv)[VEC2 ? 2 : 1],
					      const u64 *A0, const u64 *A1, int n, int G, int sub, int cj, const ModP &m)
{
	constexpr int V = VEC2 ? 2 : 1;
	const u64 xlo = xv[0], xhi = xv[V - 1];
	int i = 0;
	while (i < n) {
		if (cnt == chunk) {
			cnt = 0;
#pragma unroll
			for (int o = 0; o < 2; o++)
#pragma unroll
				for (int k = 0; k < V; k++)
					acc_set(acc[o][k], acc_reduce<MERS>(acc[o][k], m));
		}
		const u32 room = chunk - cnt, left = (u32)(n - i), run = left < room ? left : room;
		const int end = i + (int)run;
		cnt += run;
		Combine2Step<VEC2> f, h;
		for (; i + 1 < end; i += 2) {
			combine2_fetch<VEC2, H0, H1, GLB>(f, i, xlo, xhi, A0, A1, n, G, sub, cj);
			combine2_fetch<VEC2, H0, H1, GLB>(h, i + 1, xlo, xhi, A0, A1, n, G, sub, cj);
			combine2_mac<VEC2, H0, H1>(acc, f);
			combine2_mac<VEC2, H0, H1>(acc, h);
		}
		if (i < end) {
			combine2_fetch<VEC2, H0, H1, GLB>(f, i, xlo, xhi, A0, A1, n, G, sub, cj);
			combine2_mac<VEC2, H0, H1>(acc, f);
			i++;
		}
	}
}

/* a lane group of (1 << lg) lanes per row; a lane owns column `col` (VEC2: columns 2 col and 2 col + 1) of both outputs.  An
 * accumulator takes at most one product per step of the count, whichever terms enter its output: the chunk rule holds for
 * each, over all terms. */
template <bool NARROW, int MERS, bool VEC2, int BLK>
__global__ void __launch_bounds__(BLK)
k_dev_combine2(Combine2Args g, int nterms, u64 *z0, long long ldz0, u64 *z1, long long ldz1, long long rows, int n, int lg, ModP m)
{
	using A = typename std::conditional<NARROW, AccS, AccL>::type;
	constexpr int V = VEC2 ? 2 : 1;
	extern __shared__ __attribute__((aligned(16))) u64 As[];	/* [slot][i * n + j] */
	const int nn = n * n;
	for (int t = 0; t < nterms; t++) {
		int slot = pick4(t, g.where[0], g.where[1], g.where[2], g.where[3]);
		if (slot < 0)
			continue;
		for (int o = 0; o < 2; o++) {
			const u64 *src = o ? pick4(t, g.a[1][0], g.a[1][1], g.a[1][2], g.a[1][3]) : pick4(t, g.a[0][0], g.a[0][1], g.a[0][2], g.a[0][3]);
			if (src) {
				for (int k = threadIdx.x; k < nn; k += blockDim.x)
					As[slot * nn + k] = src[k];
				slot++;
			}
		}
	}
	__syncthreads();
	const int G = 1 << lg, lane = threadIdx.x & 63, col = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg;
	const int units = VEC2 ? n >> 1 : n, wpb = blockDim.x >> 6;
	const int cj = col < units ? col : 0;	/* an idle lane multiplies column 0 and stores nothing */
	const u32 chunk = NARROW ? 0x80000000u : m.chunk;
	const long long groups = (rows + rpw - 1) / rpw;
	for (long long grp = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); grp < groups; grp += (long long)gridDim.x * wpb) {
		const long long row = grp * rpw + sub;
		const bool mine = row < rows && col < units;
		u64 xv[DEVALG_MAX_TERMS][V];
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
		A acc[2][V];
#pragma unroll
		for (int o = 0; o < 2; o++)
#pragma unroll
			for (int k = 0; k < V; k++)
				acc_zero(acc[o][k]);
		u32 cnt = 0;
		for (int t = 0; t < nterms; t++) {	/* not unrolled: one body per form, the term's words and panels by selects */
			u64 xt[V];
#pragma unroll
			for (int k = 0; k < V; k++)
				xt[k] = pick4(t, xv[0][k], xv[1][k], xv[2][k], xv[3][k]);
			const u64 *G0 = pick4(t, g.a[0][0], g.a[0][1], g.a[0][2], g.a[0][3]);
			const u64 *G1 = pick4(t, g.a[1][0], g.a[1][1], g.a[1][2], g.a[1][3]);
			const bool h0 = G0 != nullptr, h1 = G1 != nullptr;
			const int slot = pick4(t, g.where[0], g.where[1], g.where[2], g.where[3]);
			if (slot < 0) {
				if (h0 && h1)
					combine2_term<MERS, VEC2, true, true, true>(acc, cnt, chunk, xt, G0, G1, n, G, sub, cj, m);
				else if (h0)
					combine2_term<MERS, VEC2, true, false, true>(acc, cnt, chunk, xt, G0, nullptr, n, G, sub, cj, m);
				else
					combine2_term<MERS, VEC2, false, true, true>(acc, cnt, chunk, xt, nullptr, G1, n, G, sub, cj, m);
			} else {
				const u64 *A0 = As + slot * nn, *A1 = As + (slot + (h0 ? 1 : 0)) * nn;
				if (h0 && h1)
					combine2_term<MERS, VEC2, true, true, false>(acc, cnt, chunk, xt, A0, A1, n, G, sub, cj, m);
				else if (h0)
					combine2_term<MERS, VEC2, true, false, false>(acc, cnt, chunk, xt, A0, nullptr, n, G, sub, cj, m);
				else
					combine2_term<MERS, VEC2, false, true, false>(acc, cnt, chunk, xt, nullptr, A1, n, G, sub, cj, m);
			}
		}
		if (mine) {
			if constexpr (VEC2) {
				*reinterpret_cast<ulonglong2 *>(z0 + row * ldz0 + 2 * col) =
					make_ulonglong2(acc_reduce<MERS>(acc[0][0], m), acc_reduce<MERS>(acc[0][1], m));
				*reinterpret_cast<ulonglong2 *>(z1 + row * ldz1 + 2 * col) =
					make_ulonglong2(acc_reduce<MERS>(acc[1][0], m), acc_reduce<MERS>(acc[1][1], m));
			} else {
				z0[row * ldz0 + col] = acc_reduce<MERS>(acc[0][0], m);
				z1[row * ldz1 + col] = acc_reduce<MERS>(acc[1][0], m);
			}
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
void dot2_go(bool v2, unsigned grid, hipStream_t s, const Dot2Args &g, long long rows, int n, int lg, const ModP &m, u64 *partial)
{
	if (v2)
		hipLaunchKernelGGL((k_dev_dot2<NARROW, MERS, NP, TT, true>), dim3(grid), dim3(BLOCK), 0, s, g, rows, n, lg, m, partial);
	else
		hipLaunchKernelGGL((k_dev_dot2<NARROW, MERS, NP, TT, false>), dim3(grid), dim3(BLOCK), 0, s, g, rows, n, lg, m, partial);
}

template <bool NARROW, int MERS>
void dot2_np(int np, bool v2, unsigned grid, hipStream_t s, const Dot2Args &g, long long rows, int n, int lg, const ModP &m,
	     u64 *partial)
{
	if (np == 1 && n == 1)
		dot2_go<NARROW, MERS, 1, 1>(v2, grid, s, g, rows, n, lg, m, partial);
	else if (np == 1)
		dot2_go<NARROW, MERS, 1, 2>(v2, grid, s, g, rows, n, lg, m, partial);
	else if (np == 4)
		dot2_go<NARROW, MERS, 4, 1>(v2, grid, s, g, rows, n, lg, m, partial);
	else if constexpr (NARROW || MERS != 0)	/* (dev_dot2_fused: the Barrett class does not come here) */
		dot2_go<NARROW, MERS, 16, 1>(v2, grid, s, g, rows, n, lg, m, partial);
}

template <bool NARROW, int MERS, bool VEC2, int BLK>
void combine2_go(unsigned grid, size_t lds, hipStream_t s, const Combine2Args &g, int nterms, u64 *z0, long long ldz0, u64 *z1,
		 long long ldz1, long long rows, int n, int lg, const ModP &m)
{
	if (lds > 48 * 1024)
		(void)hipFuncSetAttribute((const void *)k_dev_combine2<NARROW, MERS, VEC2, BLK>, hipFuncAttributeMaxDynamicSharedMemorySize,
					  (int)lds);
	hipLaunchKernelGGL((k_dev_combine2<NARROW, MERS, VEC2, BLK>), dim3(grid), dim3(BLK), lds, s, g, nterms, z0, ldz0, z1, ldz1, rows,
			   n, lg, m);
}

/* the forms that exist: 256 threads in every lane form; 1024 threads (128 registers a lane) in the 16-byte lane form only where
 * the accumulators are the 96-bit ones -- four 160-bit AccL, the rows of four terms and a pair of panel words do not fit there */
template <bool NARROW, int MERS>
void combine2_v(bool v2, unsigned grid, unsigned block, size_t lds, hipStream_t s, const Combine2Args &g, int nterms, u64 *z0,
		long long ldz0, u64 *z1, long long ldz1, long long rows, int n, int lg, const ModP &m)
{
	if (block == BLOCK) {
		if (v2)
			combine2_go<NARROW, MERS, true, BLOCK>(grid, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, m);
		else
			combine2_go<NARROW, MERS, false, BLOCK>(grid, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, m);
	} else {
		if constexpr (NARROW) {
			if (v2) {
				combine2_go<NARROW, MERS, true, 1024>(grid, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, m);
				return;
			}
		}
		combine2_go<NARROW, MERS, false, 1024>(grid, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, m);
	}
}

}  // namespace

int dev_dot2_max_blocks(const KernelCfg &c, int n)
{
	return dev_dot_max_blocks(c, n);
}

int dev_dot2_fused(const KernelCfg &c, int n)
{
	return n <= DOT2_BARRETT_MAX_N || c.m.p < (1ull << 32) || c.mers == 61 ? 1 : 0;
}

hipError_t launch_dev_dot2(const KernelCfg &c, int n, long long rows, const u64 *x0, long long ldx0, const u64 *x1, long long ldx1,
			   const u64 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s)
{
	if (n < 1 || n > 64 || rows < 0)
		return hipErrorInvalidValue;
	const int words = n * n;
	if (!dev_dot2_fused(c, n)) {	/* stream order makes the one scratch safe for both */
		const hipError_t e = launch_dev_dot(c, n, rows, x0, ldx0, y, ldy, partial, out, s);
		return e != hipSuccess ? e : launch_dev_dot(c, n, rows, x1, ldx1, y, ldy, partial, out + words, s);
	}
	const int lg = log2_ceil(n), TR = TILE_WORDS >> lg;
	const long long ntiles = (rows + TR - 1) / TR, cap = dev_dot2_max_blocks(c, n);
	const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
	if (grid) {
		Dot2Args g{};
		const u64 *ptr[3] = { y, x0, x1 };	/* Y first: it is block 0 whatever else coincides */
		const long long ld[3] = { ldy, ldx0, ldx1 };
		int idx[3] = { 0, 0, 0 };
		bool v2 = true;
		for (int k = 0; k < 3; k++) {
			int at = -1;
			for (int b = 0; b < g.nblk; b++)
				if (g.b[b] == ptr[k] && g.ld[b] == ld[k])
					at = b;
			if (at < 0) {
				at = g.nblk++;
				g.b[at] = ptr[k];
				g.ld[at] = ld[k];
				v2 = v2 && pair_ok(ptr[k], ld[k], n);
			}
			idx[k] = at;
		}
		g.iy = idx[0];
		g.ix0 = idx[1];
		g.ix1 = idx[2];
		const int np = words <= BLOCK ? 1 : words <= 4 * BLOCK ? 4 : 16;
		const bool narrow = c.m.p < (1ull << 32);
		if (narrow && c.mers == 31)
			dot2_np<true, 31>(np, v2, grid, s, g, rows, n, lg, c.m, partial);
		else if (narrow)
			dot2_np<true, 0>(np, v2, grid, s, g, rows, n, lg, c.m, partial);
		else if (c.mers == 61)
			dot2_np<false, 61>(np, v2, grid, s, g, rows, n, lg, c.m, partial);
		else
			dot2_np<false, 0>(np, v2, grid, s, g, rows, n, lg, c.m, partial);
	}
	hipLaunchKernelGGL(k_dev_dot2_finalize, dim3((unsigned)((2 * words + 7) / 8)), dim3(BLOCK), 0, s, partial, (int)grid, 2 * words,
			   c.m.p, out);
	return hipGetLastError();
}

hipError_t launch_dev_combine2(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			       const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
			       hipStream_t s)
{
	if (n < 1 || n > 64 || nterms < 1 || nterms > DEVALG_MAX_TERMS || rows < 0)
		return hipErrorInvalidValue;
	int in0 = 0, in1 = 0;
	for (int t = 0; t < nterms; t++) {
		if (!a0[t] && !a1[t])
			return hipErrorInvalidValue;
		in0 += a0[t] != nullptr;
		in1 += a1[t] != nullptr;
	}
	if (!in0 || !in1)
		return hipErrorInvalidValue;
	if (rows == 0)
		return hipSuccess;
	Combine2Args g{};
	const size_t panel = (size_t)n * n * sizeof(u64);
	const int room = (int)(LDS_BYTES / panel);	/* panels of LDS: 5 at n = 64 */
	int used = 0;
	bool v2 = pair_ok(z0, ldz0, n) && pair_ok(z1, ldz1, n);
	for (int t = 0; t < nterms; t++) {
		g.x[t] = x[t];
		g.ldx[t] = ldx[t];
		g.a[0][t] = a0[t];
		g.a[1][t] = a1[t];
		v2 = v2 && pair_ok(x[t], ldx[t], n);
		const int need = (a0[t] != nullptr) + (a1[t] != nullptr);
		g.where[t] = used + need > room ? -1 : used;	/* a term's panels go together: into LDS, or read where they lie */
		if (g.where[t] >= 0)
			used += need;
	}
	const size_t lds = (size_t)used * panel;
	const unsigned block = lds > 40 * 1024 ? 1024 : BLOCK;	/* a workgroup per CU then: make it a full one */
	const bool narrow = c.m.p < (1ull << 32);
	if (block == 1024 && !narrow)
		v2 = false;	/* (combine2_v: that form does not exist) */
	const int lg = log2_ceil(v2 ? n / 2 : n), rpw = 64 >> lg;
	const long long wpb = block / 64, groups = (rows + rpw - 1) / rpw, want = (groups + wpb - 1) / wpb;
	const long long cap = (long long)c.num_cu * (block == 1024 ? 1 : 8);
	const unsigned grid = (unsigned)(want < cap ? want : cap);
	if (narrow && c.mers == 31)
		combine2_v<true, 31>(v2, grid, block, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, c.m);
	else if (narrow)
		combine2_v<true, 0>(v2, grid, block, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, c.m);
	else if (c.mers == 61)
		combine2_v<false, 61>(v2, grid, block, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, c.m);
	else
		combine2_v<false, 0>(v2, grid, block, lds, s, g, nterms, z0, ldz0, z1, ldz1, rows, n, lg, c.m);
	return hipGetLastError();
}
