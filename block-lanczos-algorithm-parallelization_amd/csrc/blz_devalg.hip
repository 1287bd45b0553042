/*
 * blz_devalg.hip -- device block algebra: the two dense parts of a Krylov step on a caller's blocks in device memory,
 *     k_dev_dot        C_k = X_k^T * Y mod p, k < 1 or 2                       (n x n panels out of two or three tall blocks)
 *     k_dev_combine    Z = sum_t X_t * A_t mod p                               (row-local, up to four terms, in place allowed)
 *     k_dev_combine2   Z0 = sum_t X_t * A0_t, Z1 = sum_t X_t * A1_t mod p      (the same for two outputs in ONE pass)
 * A block is rows x n u64 words with a row stride of ld >= n words; the words n .. ld-1 of a row are never touched.  The
 * operations are invariant under a permutation of the rows, so unlike blz_apply_device nothing is imported into a slab: the
 * kernels stream the caller's rows where they lie.  Sums of 64 x 64 -> 128-bit products are kept unreduced for at most
 * ModP::chunk products per accumulator (modp.h: 1 at p = 2^62 - 57, 32 at 2^61 - 1; the 96-bit AccS of p < 2^32 takes 2^32 of
 * them and is reduced every 2^31), and every word written is the canonical residue of the exact integer sum.
 *
 * k_dev_dot.  Tiles of TR = 1024 >> lg consecutive rows (lg = log2 of the next power of two >= n: 128 rows at n = 8, 16 at
 * n = 64) go round-robin over the workgroups.  Blocks that are the same pointer with the same stride are ONE block
 * (dev_same_blocks): the launcher passes the distinct blocks (one to three) and which of them the X_k and Y are, and a tile of
 * 1024 words of each distinct block is staged through LDS (8 KB each), loaded by lane groups of one row each -- contiguous
 * 8-byte or, where pointer, stride and width allow, 16-byte lane accesses -- and the loads of the next tile are issued into
 * registers before the current one is multiplied.  An LDS row is padded with zeros to the power of two.  For n > 16 a thread
 * owns the entries e = t, t + 256, ... of every C_k (i = e / n from X_k, j = e % n from Y: adjacent lanes read adjacent words
 * of Y's row and broadcast X_k's).  For n <= 16 a thread owns a 2 x 2 tile of every C_k (two 16-byte LDS reads per four
 * products, four independent sums) and, n * n / 4 being less than 256, the threads also split the tile's rows into slices that
 * are added in LDS at the end.  With two X_k the word of Y a thread reads is multiplied into two accumulators.  Each workgroup
 * writes ONE row of nx * n * n residues ([panel][entry]) to the call's scratch and k_dev_dot_finalize adds the rows mod p: no
 * atomics, no host round trip.  At n > 32 a thread of the pair holds two sets of 16 accumulators: the 96-bit ones of p < 2^32
 * and the 128-bit ones of p = 2^61 - 1 fit the 256 registers of a lane, those of the Barrett class (one set alone takes 244) do
 * not without moving a set to the accumulation registers, so that class runs the single form twice inside the one call at those
 * widths (dot has no in-place form: that is correct).
 *
 * k_dev_combine.  The coefficient matrices sit in LDS (nterms * n * n words: 128 KB for four terms at n = 64, then one
 * workgroup of 1024 threads per CU; 256 threads otherwise).  A lane group of G lanes takes one row: every lane loads its
 * word (or pair of words) of the row of EVERY term into registers, the words reach the other lanes by shuffles, and only
 * then is the row of Z stored -- which is what makes Z = one of the X_t safe.
 *
 * k_dev_combine2 has the lane-group loop of k_dev_combine.  The coefficient panels of a term sit in LDS when they fit --
 * 160 KB hold five panels at n = 64, as one workgroup of 1024 threads with nothing else in LDS -- and the terms whose panels
 * do not fit read theirs from global memory, through the cache (32 KB each at the most, the same for every workgroup).  It is
 * ONE launch at every panel count: a lane group holds its row of every term in registers before it stores either output row,
 * which is what makes each of Z0 and Z1 = one of the X_t safe, and what a second launch would break.  Its inner loop is not
 * k_dev_combine's (run-length chunks, terms by selects): two accumulator sets leave it the registers for nothing else.
 */
#include "blz_devalg.h"
#include "blz_devhelp.h"

#include <type_traits>

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_WORDS = 1024;	/* one block's tile: (TILE_WORDS >> lg) rows of at most (1 << lg) words */
constexpr int DOT_BLOCKS = 3;		/* X0, X1 and Y, when all are distinct */
constexpr int DOT2_BARRETT_MAX_N = 32;	/* beyond: two sets of 16 Acc per thread, see above */
constexpr size_t LDS_BYTES = 160 * 1024;	/* of a CU, all of which one workgroup may have */

/* the words of row `row` of a block a lane owns: word `col`, or (VEC2) words 2 col and 2 col + 1; zeros unless `live` */
template <bool VEC2>
__device__ __forceinline__ void row_load(u64 (&w)[VEC2 ? 2 : 1], const u64 *b, long long ld, long long row, int col, bool live)
{
	if constexpr (VEC2) {
		ulonglong2 v = make_ulonglong2(0, 0);
		if (live)
			v = *reinterpret_cast<const ulonglong2 *>(b + row * ld + 2 * col);
		w[0] = v.x;
		w[1] = v.y;
	} else {
		w[0] = live ? b[row * ld + col] : 0;
	}
}

/* the same words of row `row` from a lane that is live */
template <bool VEC2>
__device__ __forceinline__ void row_store(u64 *b, long long ld, long long row, int col, const u64 (&w)[VEC2 ? 2 : 1])
{
	if constexpr (VEC2)
		*reinterpret_cast<ulonglong2 *>(b + row * ld + 2 * col) = make_ulonglong2(w[0], w[1]);
	else
		b[row * ld + col] = w[0];
}

/* the words of a tile a thread moves: 4 rows of one word, or 2 rows of two words */
template <bool VEC2>
struct TileRegs {
	u64 w[VEC2 ? 2 : 4][VEC2 ? 2 : 1];
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
		row_load<VEC2>(g.w[k], b, ld, row, lane, lane < units && row < rows);
	}
}

/* the same words into the LDS tile, (1 << lg) words per row: the columns past n and the rows past the block's end arrive
 * as zeros (the lanes of a row cover the whole pitch, a dead lane's registers are zero) */
template <bool VEC2>
__device__ __forceinline__ void tile_store(const TileRegs<VEC2> &g, u64 *tile, int pitch, int lgu)
{
	const int lane = threadIdx.x & ((1 << lgu) - 1), rsub = threadIdx.x >> lgu, rpp = BLOCK >> lgu;
#pragma unroll
	for (int k = 0; k < (VEC2 ? 2 : 4); k++)
		row_store<VEC2>(tile, pitch, rsub + k * rpp, lane, g.w[k]);
}

/* the distinct blocks of a call, and which of them the X_k and Y are.  The two arities keep the shapes their kernels had before
 * they were one, because each was timed faster in its own: with one X (NX = 1) X is block 0 whatever Y is, so its tile has a
 * compile-time place in LDS and its staging is under no run-time branch; with two (NX = 2) Y is block 0, every block is staged
 * under `k < nblk` and all three tile bases come from this table. */
struct DotArgs {
	const u64 *b[DOT_BLOCKS];
	long long ld[DOT_BLOCKS];
	int nblk, ix[2], iy;
};

/* NX = 1 or 2 products against Y; acc[k] belongs to C_k = X_k^T Y, and all take one product per row, so one count serves the
 * chunk rule.
 * NP = entries of a C_k per thread for n > 16: 4 (n <= 32) or 16 (n <= 64), entries t, t + 256, ...
 * NP == 1 is n <= 16: a thread owns a TT x TT tile of every C_k (TT = 2; 1 at n = 1) -- two 16-byte LDS reads per four
 * products and four independent sums -- and the 256 / (pitch / TT)^2 slices of threads split the tile's rows. */
template <bool NARROW, int MERS, int NP, int TT, bool VEC2, int NX>
__global__ void __launch_bounds__(BLOCK)
k_dev_dot(DotArgs g, long long rows, int n, int lg, ModP m, u64 *__restrict__ partial)
{
	using A = typename std::conditional<NARROW, AccS, typename std::conditional<(NP <= 4), AccL, Acc>::type>::type;
	constexpr int NACC = NP == 1 ? TT * TT : NP, NB = NX + 1;
	__shared__ __attribute__((aligned(16))) u64 tiles[NB * TILE_WORDS];
	const u64 *xt[NX], *yt = tiles + g.iy * TILE_WORDS;
	if constexpr (NX == 1) {
		xt[0] = tiles;
	} else {
#pragma unroll
		for (int k = 0; k < NX; k++)
			xt[k] = tiles + g.ix[k] * TILE_WORDS;
	}
	const int t = threadIdx.x, pairs = n * n, pitch = 1 << lg, TR = TILE_WORDS >> lg;
	const int units = VEC2 ? n >> 1 : n, lgu = VEC2 ? lg - 1 : lg;
	const int tpr = pitch / TT, tps = tpr * tpr;	/* NP == 1: tiles per row and column of a panel, threads per slice */
	const int slices = NP == 1 ? BLOCK / tps : 1, slice = NP == 1 ? t / tps : 0;
	const u32 chunk = NARROW ? 0x80000000u : m.chunk;
	A acc[NX][NACC];
	int xi[NP], yj[NP];
#pragma unroll
	for (int k = 0; k < NX; k++)
#pragma unroll
		for (int q = 0; q < NACC; q++)
			acc_zero(acc[k][q]);
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
	/* block k is there; written so that block 0 of the single form is under no run-time branch (DotArgs) */
	auto staged = [&](int k) { return (NX == 1 && k == 0) || k < g.nblk; };
	u32 cnt = 0;
	const long long ntiles = (rows + TR - 1) / TR;
	long long tile = blockIdx.x;
	TileRegs<VEC2> gr[NB];
	if (tile < ntiles) {
#pragma unroll
		for (int k = 0; k < NB; k++)
			if (staged(k))
				tile_load<VEC2>(gr[k], g.b[k], g.ld[k], tile * TR, rows, units, lgu);
	}
	while (tile < ntiles) {
		__syncthreads();	/* the tile before this one has been read */
#pragma unroll
		for (int k = 0; k < NB; k++)
			if (staged(k))
				tile_store<VEC2>(gr[k], tiles + k * TILE_WORDS, pitch, lgu);
		__syncthreads();
		const long long next = tile + gridDim.x;
		if (next < ntiles) {	/* in flight while this tile is multiplied */
#pragma unroll
			for (int k = 0; k < NB; k++)
				if (staged(k))
					tile_load<VEC2>(gr[k], g.b[k], g.ld[k], next * TR, rows, units, lgu);
		}
		const long long left = rows - tile * TR;
		const int tr = left < TR ? (int)left : TR;
		for (int r = slice; r < tr; r += slices) {
			const u64 *xr[NX], *yr = yt + r * pitch;
#pragma unroll
			for (int k = 0; k < NX; k++)
				xr[k] = xt[k] + r * pitch;
			if constexpr (NP == 1 && TT == 2) {
				ulonglong2 xa[NX];
#pragma unroll
				for (int k = 0; k < NX; k++)
					xa[k] = *reinterpret_cast<const ulonglong2 *>(xr[k] + xi[0]);
				const ulonglong2 ya = *reinterpret_cast<const ulonglong2 *>(yr + yj[0]);
#pragma unroll
				for (int k = 0; k < NX; k++) {
					acc_mac64(acc[k][0], xa[k].x, ya.x);
					acc_mac64(acc[k][1], xa[k].x, ya.y);
					acc_mac64(acc[k][2], xa[k].y, ya.x);
					acc_mac64(acc[k][3], xa[k].y, ya.y);
				}
			} else {
#pragma unroll
				for (int q = 0; q < NP; q++) {
					const u64 yv = yr[yj[q]];
#pragma unroll
					for (int k = 0; k < NX; k++)
						acc_mac64(acc[k][q], xr[k][xi[q]], yv);
				}
			}
			if (++cnt == chunk) {
				cnt = 0;
#pragma unroll
				for (int q = 0; q < NACC; q++)
#pragma unroll
					for (int k = 0; k < NX; k++)
						acc_set(acc[k][q], acc_reduce<MERS>(acc[k][q], m));
			}
		}
		tile = next;
	}
	u64 *out = partial + (size_t)blockIdx.x * NX * pairs;
	if constexpr (NP == 1) {
		__syncthreads();	/* the tiles are free: the slices' residues, [panel][entry of the tile][thread] -- NACC * 256 <= 1024 words a panel */
#pragma unroll
		for (int k = 0; k < NX; k++)
#pragma unroll
			for (int q = 0; q < NACC; q++)
				tiles[k * TILE_WORDS + q * BLOCK + t] = acc_reduce<MERS>(acc[k][q], m);
		__syncthreads();
		if (t < pairs) {
			const int i = t / n, j = t % n;
#pragma unroll
			for (int k = 0; k < NX; k++) {
				const u64 *mine = tiles + k * TILE_WORDS + ((i % TT) * TT + (j % TT)) * BLOCK + (i / TT) * tpr + (j / TT);
				u64 sum = 0;
				for (int sl = 0; sl < slices; sl++)
					sum = addmod(sum, mine[sl * tps], m.p);
				out[k * pairs + t] = sum;
			}
		}
	} else {
#pragma unroll
		for (int q = 0; q < NP; q++) {
			const int e = t + q * BLOCK;
			if (e < pairs) {
#pragma unroll
				for (int k = 0; k < NX; k++)
					out[k * pairs + e] = acc_reduce<MERS>(acc[k][q], m);
			}
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
	constexpr int V = VEC2 ? 2 : 1;
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
		u64 xv[DEVALG_MAX_TERMS][V];
#pragma unroll
		for (int t = 0; t < DEVALG_MAX_TERMS; t++)	/* the whole row of every term, before anything is stored */
			row_load<VEC2>(xv[t], g.x[t], g.ldx[t], row, col, mine && t < nterms);
		A acc[V];
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
			u64 w[V];
#pragma unroll
			for (int k = 0; k < V; k++)
				w[k] = acc_reduce<MERS>(acc[k], m);
			row_store<VEC2>(z, ldz, row, col, w);
		}
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
		for (int t = 0; t < DEVALG_MAX_TERMS; t++)	/* the whole row of every term, before anything is stored */
			row_load<VEC2>(xv[t], g.x[t], g.ldx[t], row, col, mine && t < nterms);
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
			u64 w[V];
#pragma unroll
			for (int k = 0; k < V; k++)
				w[k] = acc_reduce<MERS>(acc[0][k], m);
			row_store<VEC2>(z0, ldz0, row, col, w);
#pragma unroll
			for (int k = 0; k < V; k++)
				w[k] = acc_reduce<MERS>(acc[1][k], m);
			row_store<VEC2>(z1, ldz1, row, col, w);
		}
	}
}

/* 16-byte lane accesses: an even width, an even stride and a 16-byte aligned base */
inline bool pair_ok(const void *b, long long ld, int n)
{
	return (n & 1) == 0 && (ld & 1) == 0 && ((uintptr_t)b & 15) == 0;
}

/* reducer class of the 64-bit kernels: f(BoolTag<NARROW>, IntTag<MERS>) for <true, 31>, <true, 0>, <false, 61>, <false, 0>;
 * returns f's result */
template <typename F> DISPATCH_INLINE auto with_dev_reducer(const KernelCfg &c, F &&f)
{
	if (c.m.p < (1ull << 32))
		return c.mers == 31 ? f(BoolTag<true>{}, IntTag<31>{}) : f(BoolTag<true>{}, IntTag<0>{});
	return c.mers == 61 ? f(BoolTag<false>{}, IntTag<61>{}) : f(BoolTag<false>{}, IntTag<0>{});
}

/* 1 where the pair at width n runs k_dev_dot<..., 2>, 0 where launch_dev_dot issues the single form twice */
inline bool dot_pair_fused(const KernelCfg &c, int n)
{
	return n <= DOT2_BARRETT_MAX_N || c.m.p < (1ull << 32) || c.mers == 61;
}

template <bool NARROW, int MERS, int NP, int TT>
void dot_go(int nx, bool v2, unsigned grid, hipStream_t s, const DotArgs &g, long long rows, int n, int lg, const ModP &m, u64 *partial)
{
	auto go = [&](auto vec2, auto nxs) {
		hipLaunchKernelGGL((k_dev_dot<NARROW, MERS, NP, TT, decltype(vec2)::value, decltype(nxs)::value>), dim3(grid), dim3(BLOCK), 0,
				   s, g, rows, n, lg, m, partial);
	};
	if (nx == 1)
		v2 ? go(BoolTag<true>{}, IntTag<1>{}) : go(BoolTag<false>{}, IntTag<1>{});
	else if constexpr (NP < 16 || NARROW || MERS != 0)	/* (dot_pair_fused: the Barrett class does not come here at n > 32) */
		v2 ? go(BoolTag<true>{}, IntTag<2>{}) : go(BoolTag<false>{}, IntTag<2>{});
}

template <bool NARROW, int MERS>
void dot_np(int np, int nx, bool v2, unsigned grid, hipStream_t s, const DotArgs &g, long long rows, int n, int lg, const ModP &m,
	    u64 *partial)
{
	if (np == 1 && n == 1)
		dot_go<NARROW, MERS, 1, 1>(nx, v2, grid, s, g, rows, n, lg, m, partial);
	else if (np == 1)
		dot_go<NARROW, MERS, 1, 2>(nx, v2, grid, s, g, rows, n, lg, m, partial);
	else if (np == 4)
		dot_go<NARROW, MERS, 4, 1>(nx, v2, grid, s, g, rows, n, lg, m, partial);
	else
		dot_go<NARROW, MERS, 16, 1>(nx, v2, grid, s, g, rows, n, lg, m, partial);
}

/* threads of a recombination's workgroup, the lane form it runs in, the lane group of a row (log2) and the grid.  Past 40 KB
 * of LDS a workgroup has a CU to itself: make it a full one.  v2: the blocks allow 16-byte lanes; v2_at_1024: that form
 * exists at 1024 threads. */
struct CombineShape {
	unsigned block, grid;
	int lg;
	bool v2;
};
inline CombineShape combine_shape(const KernelCfg &c, long long rows, int n, size_t lds, bool v2, bool v2_at_1024)
{
	const unsigned block = lds > 40 * 1024 ? 1024 : BLOCK;
	v2 = v2 && (block == BLOCK || v2_at_1024);
	const int lg = log2_ceil(v2 ? n / 2 : n), rpw = 64 >> lg;
	const long long wpb = block / 64, groups = (rows + rpw - 1) / rpw, want = (groups + wpb - 1) / wpb;
	const long long cap = (long long)c.num_cu * (block == 1024 ? 1 : 8);
	return CombineShape{ block, (unsigned)(want < cap ? want : cap), lg, v2 };
}

hipError_t combine1(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
		    const u64 *const *a, u64 *z, long long ldz, hipStream_t s)
{
	CombineArgs g{};
	bool v2 = pair_ok(z, ldz, n);
	for (int t = 0; t < nterms; t++) {
		g.x[t] = x[t];
		g.ldx[t] = ldx[t];
		g.a[t] = a[t];
		v2 = v2 && pair_ok(x[t], ldx[t], n);
	}
	const size_t lds = (size_t)nterms * n * n * sizeof(u64);
	const CombineShape sh = combine_shape(c, rows, n, lds, v2, true);
	return with_dev_reducer(c, [&](auto narrow, auto mers) {
		auto go = [&](auto vec2) {
			constexpr auto K = &k_dev_combine<decltype(narrow)::value, decltype(mers)::value, decltype(vec2)::value>;
			const hipError_t e = dev_lds_limit<K>(lds, DEVALG_MAX_TERMS * 64 * 64 * sizeof(u64));
			if (e != hipSuccess)
				return e;
			hipLaunchKernelGGL(K, dim3(sh.grid), dim3(sh.block), lds, s, g, nterms, z, ldz, rows, n, sh.lg, c.m);
			return hipGetLastError();
		};
		return sh.v2 ? go(BoolTag<true>{}) : go(BoolTag<false>{});
	});
}

hipError_t combine2(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
		    const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1, hipStream_t s)
{
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
	/* the forms that exist: 256 threads in every lane form; 1024 threads (128 registers a lane) in the 16-byte lane form only
	 * where the accumulators are the 96-bit ones -- four 160-bit AccL, the rows of four terms and a pair of panel words do not
	 * fit there */
	const bool narrow_p = c.m.p < (1ull << 32);
	const CombineShape sh = combine_shape(c, rows, n, lds, v2, narrow_p);
	return with_dev_reducer(c, [&](auto narrow, auto mers) {
		constexpr bool NARROW = decltype(narrow)::value;
		auto go = [&](auto vec2, auto blk) {
			constexpr auto K = &k_dev_combine2<NARROW, decltype(mers)::value, decltype(vec2)::value, decltype(blk)::value>;
			const hipError_t e = dev_lds_limit<K>(lds, LDS_BYTES);
			if (e != hipSuccess)
				return e;
			hipLaunchKernelGGL(K, dim3(sh.grid), dim3((unsigned)decltype(blk)::value), lds, s, g, nterms, z0, ldz0, z1, ldz1, rows,
					   n, sh.lg, c.m);
			return hipGetLastError();
		};
		if (sh.block == BLOCK)
			return sh.v2 ? go(BoolTag<true>{}, IntTag<BLOCK>{}) : go(BoolTag<false>{}, IntTag<BLOCK>{});
		if constexpr (NARROW) {
			if (sh.v2)
				return go(BoolTag<true>{}, IntTag<1024>{});
		}
		return go(BoolTag<false>{}, IntTag<1024>{});
	});
}

}  // namespace

/* the scratch stays at 8 MB at n = 64 (256 partial rows of 32 KB) and below it elsewhere; twice that for the pair */
int dev_dot_max_blocks(const KernelCfg &c, int n)
{
	const long long by_bytes = ((long long)8 << 20) / ((long long)n * n * 8), by_cu = (long long)c.num_cu * 4;
	const long long b = by_bytes < by_cu ? by_bytes : by_cu;
	return (int)(b < 1 ? 1 : b);
}

void dev_same_blocks(int nb, const void *const *b, const long long *ld, int *first)
{
	for (int k = 0; k < nb; k++) {
		first[k] = k;
		for (int j = k - 1; j >= 0; j--)
			if (b[j] == b[k] && ld[j] == ld[k])
				first[k] = j;
	}
}

hipError_t launch_dev_dot_finalize(const u64 *partial, int nblocks, int words, u64 p, u64 *out, hipStream_t s)
{
	hipLaunchKernelGGL(k_dev_dot_finalize, dim3((unsigned)((words + 7) / 8)), dim3(BLOCK), 0, s, partial, nblocks, words, p, out);
	return hipGetLastError();
}

hipError_t launch_dev_dot(const KernelCfg &c, int n, long long rows, int nx, const u64 *const *x, const long long *ldx,
			  const u64 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s)
{
	if (n < 1 || n > 64 || rows < 0 || nx < 1 || nx > 2)
		return hipErrorInvalidValue;
	const int words = n * n;
	if (nx == 2 && !dot_pair_fused(c, n)) {	/* stream order makes the one scratch safe for both */
		const hipError_t e = launch_dev_dot(c, n, rows, 1, x, ldx, y, ldy, partial, out, s);
		return e != hipSuccess ? e : launch_dev_dot(c, n, rows, 1, x + 1, ldx + 1, y, ldy, partial, out + words, s);
	}
	const int lg = log2_ceil(n), TR = TILE_WORDS >> lg;
	const long long ntiles = (rows + TR - 1) / TR, cap = dev_dot_max_blocks(c, n);
	const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
	if (grid) {
		/* the block that is block 0 whatever else coincides goes first: X at nx = 1, Y at nx = 2 (DotArgs) */
		const int at_y = nx == 1 ? 1 : 0, at_x = 1 - at_y;
		const void *ptr[DOT_BLOCKS];
		long long ld[DOT_BLOCKS];
		ptr[at_y] = y, ld[at_y] = ldy;
		for (int k = 0; k < nx; k++)
			ptr[at_x + k] = x[k], ld[at_x + k] = ldx[k];
		int first[DOT_BLOCKS], idx[DOT_BLOCKS];
		dev_same_blocks(nx + 1, ptr, ld, first);
		DotArgs g{};
		bool v2 = true;
		for (int k = 0; k <= nx; k++) {
			if (first[k] == k) {
				idx[k] = g.nblk++;
				g.b[idx[k]] = (const u64 *)ptr[k];
				g.ld[idx[k]] = ld[k];
				v2 = v2 && pair_ok(ptr[k], ld[k], n);
			} else {
				idx[k] = idx[first[k]];
			}
		}
		g.iy = idx[at_y];
		for (int k = 0; k < nx; k++)
			g.ix[k] = idx[at_x + k];
		const int np = words <= BLOCK ? 1 : words <= 4 * BLOCK ? 4 : 16;
		with_dev_reducer(c, [&](auto narrow, auto mers) {
			dot_np<decltype(narrow)::value, decltype(mers)::value>(np, nx, v2, grid, s, g, rows, n, lg, c.m, partial);
		});
	}
	return launch_dev_dot_finalize(partial, (int)grid, nx * words, c.m.p, out, s);
}

hipError_t launch_dev_combine(const KernelCfg &c, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
			      int nz, const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
			      hipStream_t s)
{
	if (n < 1 || n > 64 || nterms < 1 || nterms > DEVALG_MAX_TERMS || rows < 0 || nz < 1 || nz > 2)
		return hipErrorInvalidValue;
	if (nz == 2) {
		int in0 = 0, in1 = 0;
		for (int t = 0; t < nterms; t++) {
			if (!a0[t] && !a1[t])
				return hipErrorInvalidValue;
			in0 += a0[t] != nullptr;
			in1 += a1[t] != nullptr;
		}
		if (!in0 || !in1)
			return hipErrorInvalidValue;
	}
	if (rows == 0)
		return hipSuccess;
	return nz == 1 ? combine1(c, n, rows, nterms, x, ldx, a0, z0, ldz0, s)
		       : combine2(c, n, rows, nterms, x, ldx, a0, a1, z0, ldz0, z1, ldz1, s);
}
