/*
 * blz_devw32.hip -- the device-block family on a caller's blocks of 32-bit words (p < 2^32, the reference's own domain):
 *     k_w32_import / k_w32_export   the caller's u32 rows (file numbering, stride ld) <-> the solver's 4-byte slab
 *     k_w32_dot                     C_k = X_k^T * Y mod p, k < 1 or 2      (blz_dot_device32, blz_dot_pair_device32)
 *     k_w32_combine                 Z_o = sum_t X_t * A_o,t mod p, o < 1 or 2 (blz_combine_device32, blz_combine_pair_device32)
 * A block is rows x n u32 residues with a row stride of ld >= n words; the words n .. ld-1 of a row are never touched.  The
 * n x n operands stay u64 words.  Every sum is the 96-bit AccS of modp.h (one v_mad_u64_u32 and one carry per product) and
 * every word written is the canonical residue of the exact integer sum, so the words are those of the 64-bit namesakes.
 *
 * Lane accesses.  A lane moves V = 4, 2 or 1 words (16, 8 or 4 bytes) of a caller's row at a time.  V is chosen per block by
 * dev_w32_width() -- n and ld multiples of V and the base aligned to 4 V bytes -- and a call runs at the least V of its blocks,
 * so an odd n, an odd ld or a base that is only 4-byte aligned go through the narrower forms.  Because V divides n a vector
 * access never reaches the words n .. ld-1.
 *
 * k_w32_import / k_w32_export walk the slab rows in order like blz_devio.hip: a lane group of the next power of two >= the
 * row's units per slab row, the caller's side a gather / scatter of whole rows through inv.  V > 1 also needs un == np.
 *
 * k_w32_dot.  Tiles of TR = 2048 >> lg consecutive rows (lg = ceil(log2 n): 256 rows at n = 8, 32 at n = 64 -- twice the rows
 * of the u64 kernel in the same 8 KB of LDS per block) go round-robin over the workgroups.  The tiles of the 2 or 3 blocks are
 * staged through LDS as u32 words, blocks that are the same pointer and stride once, and the loads of the next tile are issued
 * into registers (8 words per thread and block) before the current one is multiplied.  A thread owns a TT x TT tile of every
 * C_k: TT = 4 for n > 16 (two 16-byte LDS reads per 16 products), 2 for n <= 16, 1 at n = 1; where (pitch / TT)^2 is less than
 * 256 the threads also split the tile's rows into slices, which are added in LDS at the end (as u32 residues).  Each workgroup
 * writes ONE row of canonical u64 residues to the scratch of the 64-bit namesake and k_dev_dot_finalize adds the rows mod p: no
 * atomics.  AccS takes 2^32 products of residues below 2^32; a counter reduces it every 2^31.
 *
 * k_w32_combine.  The coefficient matrices are narrowed to u32 on their way into LDS ([output][term][n * n]: 64 KB for four
 * terms at n = 64, 128 KB for the pair).  A lane group takes one row: every lane loads its V words of the row of EVERY term
 * into registers, the words reach the other lanes by shuffles, and only then are the rows of the outputs stored -- which is
 * what makes an output that IS one of the X_t safe.  A sum has at most 4 * 64 products: no cadence is needed.
 */
#include "blz_devw32.h"
#include "blz_devhelp.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAXB = 3;		/* blocks of an inner product: x0, x1, y */

template <int V>
__device__ __forceinline__ void load_words(u32 (&w)[V], const u32 *p)
{
	if constexpr (V == 4) {
		const uint4 t = *reinterpret_cast<const uint4 *>(p);
		w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
	} else if constexpr (V == 2) {
		const uint2 t = *reinterpret_cast<const uint2 *>(p);
		w[0] = t.x, w[1] = t.y;
	} else {
		w[0] = *p;
	}
}

template <int V>
__device__ __forceinline__ void store_words(u32 *p, const u32 (&w)[V])
{
	if constexpr (V == 4)
		*reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
	else if constexpr (V == 2)
		*reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
	else
		*p = w[0];
}

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
	for (int off = 32; off > 0; off >>= 1)
		v += __shfl_xor(v, off, 64);
	return v;
}

/* ---------------------------------------------------------------------------------------------------- import / export */

/* COUNT: the words that are not below p are counted, one atomic per wavefront that saw any.  V > 1: un == np */
template <int V, bool COUNT>
__global__ void __launch_bounds__(BLOCK) k_w32_import(u32 *__restrict__ slab, const u32 *__restrict__ caller, long long ld,
						       const int *__restrict__ inv, long long rows, int un, int np, int lg, u32 p,
						       unsigned long long *bad)
{
	const int lane = threadIdx.x & ((1 << lg) - 1), rpb = BLOCK >> lg;
	const int units = np / V;
	unsigned long long cnt = 0;
	if (lane < units)
		for (long long s = (long long)blockIdx.x * rpb + (threadIdx.x >> lg); s < rows; s += (long long)gridDim.x * rpb) {
			const long long o = inv ? (long long)inv[s] : s;
			u32 w[V];
			if constexpr (V == 1)
				w[0] = lane < un ? caller[o * ld + lane] : 0;
			else
				load_words<V>(w, caller + o * ld + V * lane);
			store_words<V>(slab + s * np + V * lane, w);
			if (COUNT)
#pragma unroll
				for (int k = 0; k < V; k++)
					cnt += w[k] >= p;
		}
	if (COUNT) {
		cnt = wave_sum(cnt);
		if ((threadIdx.x & 63) == 0 && cnt)
			atomicAdd(bad, cnt);
	}
}

template <int V>
__global__ void __launch_bounds__(BLOCK) k_w32_export(u32 *__restrict__ caller, long long ld, const u32 *__restrict__ slab,
						       const int *__restrict__ inv, long long rows, int un, int np, int lg)
{
	const int lane = threadIdx.x & ((1 << lg) - 1), rpb = BLOCK >> lg;
	if (lane >= un / V)
		return;
	for (long long s = (long long)blockIdx.x * rpb + (threadIdx.x >> lg); s < rows; s += (long long)gridDim.x * rpb) {
		const long long o = inv ? (long long)inv[s] : s;
		u32 w[V];
		load_words<V>(w, slab + s * np + V * lane);
		store_words<V>(caller + o * ld + V * lane, w);
	}
}

/* ---------------------------------------------------------------------------------------------------- inner products */

struct DotArgs {
	const u32 *b[MAXB];	/* x0, (x1,) y */
	long long ld[MAXB];
	int slot[MAXB];		/* the first block that is the same pointer and stride: staged there, once */
};

/* rows [row0, row0 + TR) of a block into registers: a lane group of (1 << lgu) lanes per row, `units` of them live, 8 / V
 * rows per thread.  The dead lanes and the rows past the block's end hold zeros. */
template <int V>
__device__ __forceinline__ void tile_load(u32 (&g)[8], const u32 *__restrict__ b, long long ld, long long row0, long long rows,
					  int units, int lgu)
{
	const int lane = threadIdx.x & ((1 << lgu) - 1), rsub = threadIdx.x >> lgu, rpp = BLOCK >> lgu;
#pragma unroll
	for (int k = 0; k < 8 / V; k++) {
		const long long row = row0 + rsub + k * rpp;
		u32 w[V];
#pragma unroll
		for (int v = 0; v < V; v++)
			w[v] = 0;
		if (lane < units && row < rows)
			load_words<V>(w, b + row * ld + V * lane);
#pragma unroll
		for (int v = 0; v < V; v++)
			g[k * V + v] = w[v];
	}
}

/* the same words into the LDS tile, (1 << lg) words per row: the lanes of a row cover the whole pitch, so the columns past n
 * and the rows past the block's end arrive as zeros.  (8 / V) * (BLOCK >> lgu) rows = the tile's TR, V << lgu = its pitch. */
template <int V>
__device__ __forceinline__ void tile_store(const u32 (&g)[8], u32 *tile, int pitch, int lgu)
{
	const int lane = threadIdx.x & ((1 << lgu) - 1), rsub = threadIdx.x >> lgu, rpp = BLOCK >> lgu;
#pragma unroll
	for (int k = 0; k < 8 / V; k++) {
		u32 w[V];
#pragma unroll
		for (int v = 0; v < V; v++)
			w[v] = g[k * V + v];
		store_words<V>(tile + (rsub + k * rpp) * pitch + V * lane, w);
	}
}

/* NB = 2: x0, y (one panel); NB = 3: x0, x1, y (two panels).  TT <= pitch, V <= pitch. */
template <int TT, int V, int NB>
__global__ void __launch_bounds__(BLOCK) k_w32_dot(DotArgs g, long long rows, int n, int lg, ModP m, u64 *__restrict__ partial)
{
	constexpr int NX = NB - 1, NT = TT * TT;
	__shared__ __attribute__((aligned(16))) u32 lds[NB * W32_TILE_WORDS];
	const int t = threadIdx.x, pairs = n * n, pitch = 1 << lg, TR = W32_TILE_WORDS >> lg;
	const int units = n / V, lgu = lg - (V == 4 ? 2 : V == 2 ? 1 : 0);
	const int tpr = pitch / TT, tps = tpr * tpr;	/* thread tiles per row and column of C, threads per slice */
	const int slices = BLOCK / tps, slice = t / tps;
	const int xi = TT * ((t % tps) / tpr), yj = TT * ((t % tps) % tpr);
	const u32 *tx[NX], *ty = lds + g.slot[NB - 1] * W32_TILE_WORDS;
#pragma unroll
	for (int k = 0; k < NX; k++)
		tx[k] = lds + g.slot[k] * W32_TILE_WORDS;
	AccS acc[NX][NT];
#pragma unroll
	for (int k = 0; k < NX; k++)
#pragma unroll
		for (int q = 0; q < NT; q++)
			acc_zero(acc[k][q]);
	u32 cnt = 0;
	const long long ntiles = (rows + TR - 1) / TR;
	long long tile = blockIdx.x;
	u32 gw[NB][8];
	if (tile < ntiles) {
#pragma unroll
		for (int b = 0; b < NB; b++)
			if (g.slot[b] == b)
				tile_load<V>(gw[b], g.b[b], g.ld[b], tile * TR, rows, units, lgu);
	}
	while (tile < ntiles) {
		__syncthreads();	/* the tile before this one has been read */
#pragma unroll
		for (int b = 0; b < NB; b++)
			if (g.slot[b] == b)
				tile_store<V>(gw[b], lds + b * W32_TILE_WORDS, pitch, lgu);
		__syncthreads();
		const long long next = tile + gridDim.x;
		if (next < ntiles) {	/* in flight while this tile is multiplied */
#pragma unroll
			for (int b = 0; b < NB; b++)
				if (g.slot[b] == b)
					tile_load<V>(gw[b], g.b[b], g.ld[b], next * TR, rows, units, lgu);
		}
		const long long left = rows - tile * TR;
		const int tr = left < TR ? (int)left : TR;
		for (int r = slice; r < tr; r += slices) {
			u32 ya[TT];
			load_words<TT>(ya, ty + r * pitch + yj);
#pragma unroll
			for (int k = 0; k < NX; k++) {
				u32 xa[TT];
				load_words<TT>(xa, tx[k] + r * pitch + xi);
#pragma unroll
				for (int a = 0; a < TT; a++)
#pragma unroll
					for (int b = 0; b < TT; b++)
						acc_mac64(acc[k][a * TT + b], xa[a], ya[b]);
			}
			if (++cnt == 0x80000000u) {	/* the cadence of AccS: 2^31 products a sum */
				cnt = 0;
#pragma unroll
				for (int k = 0; k < NX; k++)
#pragma unroll
					for (int q = 0; q < NT; q++)
						acc_set(acc[k][q], acc_reduce<0>(acc[k][q], m));
			}
		}
		tile = next;
	}
	/* the slices' residues through LDS, [entry of the thread tile][thread]: NT * 256 u32 words <= the tiles' NB * 2048 */
	u64 *out = partial + (size_t)blockIdx.x * NX * pairs;
#pragma unroll
	for (int k = 0; k < NX; k++) {
		__syncthreads();	/* the tiles, or the panel before this one, have been read */
#pragma unroll
		for (int q = 0; q < NT; q++)
			lds[q * BLOCK + t] = (u32)acc_reduce<0>(acc[k][q], m);
		__syncthreads();
		for (int e = t; e < pairs; e += BLOCK) {
			const int i = e / n, j = e % n;
			const u32 *mine = lds + ((i % TT) * TT + (j % TT)) * BLOCK + (i / TT) * tpr + (j / TT);
			u64 s = 0;
			for (int sl = 0; sl < slices; sl++)
				s = addmod(s, (u64)mine[sl * tps], m.p);
			out[k * pairs + e] = s;
		}
	}
}

/* ---------------------------------------------------------------------------------------------------- recombinations */

struct CombineArgs {
	const u32 *x[DEVALG_MAX_TERMS];
	long long ldx[DEVALG_MAX_TERMS];
	const u64 *a[2][DEVALG_MAX_TERMS];	/* NULL: the term does not enter that output */
	u32 *z[2];
	long long ldz[2];
};

/* a lane group of (1 << lg) lanes per row; a lane owns the columns V col .. V col + V - 1 */
template <int V, int NZ>
__global__ void __launch_bounds__(1024) k_w32_combine(CombineArgs g, int nterms, long long rows, int n, int lg, ModP m)
{
	extern __shared__ __attribute__((aligned(16))) u32 As[];	/* [output][term][i * n + j] */
	const int nn = n * n;
	for (int o = 0; o < NZ; o++)
		for (int t = 0; t < nterms; t++)
			if (g.a[o][t])
				for (int k = threadIdx.x; k < nn; k += blockDim.x)
					As[(o * nterms + t) * nn + k] = (u32)g.a[o][t][k];
	__syncthreads();
	const int G = 1 << lg, lane = threadIdx.x & 63, col = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg;
	const int units = n / V, wpb = blockDim.x >> 6;
	const int cj = col < units ? col : 0;	/* an idle lane multiplies its group's first columns and stores nothing */
	const long long groups = (rows + rpw - 1) / rpw;
	for (long long grp = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); grp < groups; grp += (long long)gridDim.x * wpb) {
		const long long row = grp * rpw + sub;
		const bool mine = row < rows && col < units;
		u32 xv[DEVALG_MAX_TERMS][V];
#pragma unroll
		for (int t = 0; t < DEVALG_MAX_TERMS; t++) {	/* the whole row of every term, before anything is stored */
#pragma unroll
			for (int v = 0; v < V; v++)
				xv[t][v] = 0;
			if (mine && t < nterms)
				load_words<V>(xv[t], g.x[t] + row * g.ldx[t] + V * col);
		}
		AccS acc[NZ][V];
#pragma unroll
		for (int o = 0; o < NZ; o++)
#pragma unroll
			for (int v = 0; v < V; v++)
				acc_zero(acc[o][v]);
#pragma unroll
		for (int t = 0; t < DEVALG_MAX_TERMS; t++) {
			if (t >= nterms)
				break;
			for (int i0 = 0; i0 < n; i0 += V) {
#pragma unroll
				for (int h = 0; h < V; h++) {
					const u32 xw = (u32)__shfl((int)xv[t][h], sub * G + i0 / V, 64);
#pragma unroll
					for (int o = 0; o < NZ; o++) {
						if (!g.a[o][t])
							continue;
						u32 av[V];
						load_words<V>(av, As + (o * nterms + t) * nn + (i0 + h) * n + V * cj);
#pragma unroll
						for (int v = 0; v < V; v++)
							acc_mac64(acc[o][v], xw, av[v]);
					}
				}
			}
		}
		if (mine) {
#pragma unroll
			for (int o = 0; o < NZ; o++) {
				u32 w[V];
#pragma unroll
				for (int v = 0; v < V; v++)
					w[v] = (u32)acc_reduce<0>(acc[o][v], m);
				store_words<V>(g.z[o] + row * g.ldz[o] + V * col, w);
			}
		}
	}
}

/* ---------------------------------------------------------------------------------------------------- launchers */

/* lane group of a row (log2) and the grid: every CU a few workgroups, rows beyond them by the grid stride */
struct Shape {
	int lg;
	unsigned grid;
};
inline Shape shape_for(const KernelCfg &c, long long rows, int units)
{
	const int lg = log2_ceil(units);
	const long long rpb = BLOCK >> lg, want = (rows + rpb - 1) / rpb, cap = (long long)c.num_cu * 8;
	return Shape{ lg, (unsigned)(want < cap ? want : cap) };
}

template <int TT, int NB>
void dot_v(int v, unsigned grid, hipStream_t s, const DotArgs &g, long long rows, int n, int lg, const ModP &m, u64 *partial)
{
	if (v == 4 && TT > 1)
		hipLaunchKernelGGL((k_w32_dot<TT, (TT > 1 ? 4 : 1), NB>), dim3(grid), dim3(BLOCK), 0, s, g, rows, n, lg, m, partial);
	else if (v == 2 && TT > 1)
		hipLaunchKernelGGL((k_w32_dot<TT, (TT > 1 ? 2 : 1), NB>), dim3(grid), dim3(BLOCK), 0, s, g, rows, n, lg, m, partial);
	else
		hipLaunchKernelGGL((k_w32_dot<TT, 1, NB>), dim3(grid), dim3(BLOCK), 0, s, g, rows, n, lg, m, partial);
}

template <int NB>
void dot_tt(int v, unsigned grid, hipStream_t s, const DotArgs &g, long long rows, int n, int lg, const ModP &m, u64 *partial)
{
	if (n == 1)
		dot_v<1, NB>(v, grid, s, g, rows, n, lg, m, partial);
	else if (n <= 16)
		dot_v<2, NB>(v, grid, s, g, rows, n, lg, m, partial);
	else
		dot_v<4, NB>(v, grid, s, g, rows, n, lg, m, partial);
}

/* the most LDS an instantiation can ask for: NZ outputs x four terms x 64 x 64 u32 words */
template <int V, int NZ>
hipError_t combine_go(unsigned grid, unsigned block, size_t lds, hipStream_t s, const CombineArgs &g, int nterms, long long rows,
		      int n, int lg, const ModP &m)
{
	const hipError_t e = dev_lds_limit<&k_w32_combine<V, NZ>>(lds, NZ * DEVALG_MAX_TERMS * 64 * 64 * sizeof(u32));
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL((k_w32_combine<V, NZ>), dim3(grid), dim3(block), lds, s, g, nterms, rows, n, lg, m);
	return hipGetLastError();
}

template <int NZ>
hipError_t combine_v(int v, unsigned grid, unsigned block, size_t lds, hipStream_t s, const CombineArgs &g, int nterms,
		     long long rows, int n, int lg, const ModP &m)
{
	if (v == 4)
		return combine_go<4, NZ>(grid, block, lds, s, g, nterms, rows, n, lg, m);
	if (v == 2)
		return combine_go<2, NZ>(grid, block, lds, s, g, nterms, rows, n, lg, m);
	return combine_go<1, NZ>(grid, block, lds, s, g, nterms, rows, n, lg, m);
}

}  // namespace

int dev_w32_width(const void *block, long long ld, int n)
{
	const uintptr_t a = (uintptr_t)block;
	if ((n & 3) == 0 && (ld & 3) == 0 && (a & 15) == 0)
		return 4;
	if ((n & 1) == 0 && (ld & 1) == 0 && (a & 7) == 0)
		return 2;
	return 1;
}

int dev_w32_tile_rows(int n) { return W32_TILE_WORDS >> log2_ceil(n); }

hipError_t launch_w32_import(const KernelCfg &c, void *slab, const u32 *caller, long long ld, const int *inv, long long rows,
			     int un, unsigned long long *bad, hipStream_t s)
{
	if (c.word != 4 || un < 1 || un > c.n)
		return hipErrorInvalidValue;
	if (rows <= 0)
		return hipSuccess;
	const int np = c.n;
	const int v = un == np ? dev_w32_width(caller, ld, un) : 1;
	const Shape sh = shape_for(c, rows, np / v);
#define IMPORT(V, CNT)                                                                                                      \
	hipLaunchKernelGGL((k_w32_import<V, CNT>), dim3(sh.grid), dim3(BLOCK), 0, s, (u32 *)slab, caller, ld, inv, rows, un, np, \
			   sh.lg, (u32)c.m.p, bad)
	if (v == 4) {
		if (bad)
			IMPORT(4, true);
		else
			IMPORT(4, false);
	} else if (v == 2) {
		if (bad)
			IMPORT(2, true);
		else
			IMPORT(2, false);
	} else {
		if (bad)
			IMPORT(1, true);
		else
			IMPORT(1, false);
	}
#undef IMPORT
	return hipGetLastError();
}

hipError_t launch_w32_export(const KernelCfg &c, u32 *caller, long long ld, const void *slab, const int *inv, long long rows,
			     int un, hipStream_t s)
{
	if (c.word != 4 || un < 1 || un > c.n)
		return hipErrorInvalidValue;
	if (rows <= 0)
		return hipSuccess;
	const int np = c.n;
	const int v = un == np ? dev_w32_width(caller, ld, un) : 1;
	const Shape sh = shape_for(c, rows, un / v);
#define EXPORT(V) \
	hipLaunchKernelGGL((k_w32_export<V>), dim3(sh.grid), dim3(BLOCK), 0, s, caller, ld, (const u32 *)slab, inv, rows, un, np, sh.lg)
	if (v == 4)
		EXPORT(4);
	else if (v == 2)
		EXPORT(2);
	else
		EXPORT(1);
#undef EXPORT
	return hipGetLastError();
}

hipError_t launch_w32_dot(const KernelCfg &c, int n, long long rows, int nx, const u32 *const *x, const long long *ldx,
			  const u32 *y, long long ldy, u64 *partial, u64 *out, hipStream_t s)
{
	if (n < 1 || n > 64 || rows < 0 || nx < 1 || nx > 2 || c.m.p >= (1ull << 32))
		return hipErrorInvalidValue;
	const int lg = log2_ceil(n), TR = W32_TILE_WORDS >> lg, words = nx * n * n, nb = nx + 1;
	const long long ntiles = (rows + TR - 1) / TR, cap = dev_dot_max_blocks(c, n);
	const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
	if (grid) {
		DotArgs g{};
		const void *ptr[MAXB];
		int v = 4;
		for (int b = 0; b < nb; b++) {
			ptr[b] = g.b[b] = b < nx ? x[b] : y;
			g.ld[b] = b < nx ? ldx[b] : ldy;
			const int w = dev_w32_width(g.b[b], g.ld[b], n);
			v = w < v ? w : v;
		}
		dev_same_blocks(nb, ptr, g.ld, g.slot);
		if (nx == 1)
			dot_tt<2>(v, grid, s, g, rows, n, lg, c.m, partial);
		else
			dot_tt<3>(v, grid, s, g, rows, n, lg, c.m, partial);
	}
	return launch_dev_dot_finalize(partial, (int)grid, words, c.m.p, out, s);
}

hipError_t launch_w32_combine(const KernelCfg &c, int n, long long rows, int nterms, const u32 *const *x, const long long *ldx,
			      int nz, const u64 *const *a0, const u64 *const *a1, u32 *z0, long long ldz0, u32 *z1, long long ldz1,
			      hipStream_t s)
{
	if (n < 1 || n > 64 || nterms < 1 || nterms > DEVALG_MAX_TERMS || rows < 0 || nz < 1 || nz > 2 || c.m.p >= (1ull << 32))
		return hipErrorInvalidValue;
	if (rows == 0)
		return hipSuccess;
	CombineArgs g{};
	g.z[0] = z0, g.ldz[0] = ldz0;
	int v = dev_w32_width(z0, ldz0, n);
	if (nz == 2) {
		g.z[1] = z1, g.ldz[1] = ldz1;
		const int w = dev_w32_width(z1, ldz1, n);
		v = w < v ? w : v;
	}
	for (int t = 0; t < nterms; t++) {
		g.x[t] = x[t];
		g.ldx[t] = ldx[t];
		g.a[0][t] = a0[t];
		g.a[1][t] = nz == 2 ? a1[t] : nullptr;
		const int w = dev_w32_width(x[t], ldx[t], n);
		v = w < v ? w : v;
	}
	const int lg = log2_ceil(n / v), rpw = 64 >> lg;
	const size_t lds = (size_t)nz * nterms * n * n * sizeof(u32);
	/* past 40 KB few workgroups fit a CU: make them full ones, two where 160 KB of LDS hold two (64 KB: four terms at n = 64) */
	const unsigned block = lds > 40 * 1024 ? 1024 : BLOCK;
	const long long per_cu = block == 1024 ? (2 * lds <= 160 * 1024 ? 2 : 1) : 8;
	const long long wpb = block / 64, groups = (rows + rpw - 1) / rpw, want = (groups + wpb - 1) / wpb;
	const long long cap = (long long)c.num_cu * per_cu;
	const unsigned grid = (unsigned)(want < cap ? want : cap);
	if (nz == 1)
		return combine_v<1>(v, grid, block, lds, s, g, nterms, rows, n, lg, c.m);
	return combine_v<2>(v, grid, block, lds, s, g, nterms, rows, n, lg, c.m);
}
