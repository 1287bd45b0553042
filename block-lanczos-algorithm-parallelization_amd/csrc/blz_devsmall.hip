/*
 * blz_devsmall.hip -- device small algebra: the fourth part of a Krylov step, and the echelon form of a caller's block,
 *     k_dev_chain   semi_inverse() of an n x n matrix and, with it, the five coefficient panels of orthogonalize()
 *                   (sequential/lanczos_modp.c:342-438 and :456-475): one workgroup, ONE launch
 *     k_dev_rref    canonical RREF of the row space of rows x n u64 words at a row stride of ld words, its pivots and
 *                   the canonical null basis: a partial launch over the rows, a merge launch of one workgroup
 * Every operand is u64 words in device memory whatever the context's word size, every word written is a canonical residue,
 * and nothing of a context is read but the modulus.  All three reducer classes of modp.h (p = 2^61 - 1, p = 2^31 - 1, Barrett
 * for any other p < 2^62) run on the 128-bit accumulator, so p < 2^32 needs no form of its own.
 *
 * k_dev_chain.  The matrices sit in LDS: A (the matrix being swept), W (which becomes winv), a copy of vtav and, for the
 * coefficients, vtaav -- four n x n matrices, 128 KB at n = 64, in the dynamic region only (a static would shift its base).
 * A thread is (row of the pass, column); the workgroup has G x G threads (G = the power of two >= n), at most 1024, so a
 * column's elimination is one pass up to n = 32 and four at n = 64.  The sweep is the fraction-free Gauss-Jordan of
 * k_semi_inverse (blz_kernels.hip): row i is carried as s_i times the reference's row, the pivot rule and so d are the
 * reference's, and ONE modular inverse at the end turns the n scalars into their inverses.  The serial chain per column is
 * kept short:
 *   - every wavefront finds the pivot itself (n <= 64 rows: one LDS read and one ballot), nothing is published;
 *   - of A only the columns right of the pivot column are updated: the others are never read again.  The multiplier
 *     A[i][j] is therefore read but not written in the pass that uses it, and a column needs ONE barrier (two more when
 *     the pivot is off the diagonal and two rows are exchanged -- rare mod a large prime);
 *   - s * x + (p - f) * y is below 2 p^2 < 2^125 <= 2^(63 + k): one reduction per word at every class.
 * The coefficient products W * S are n^3 multiply-accumulates over the whole workgroup with the chunk rule of modp.h.
 *
 * k_dev_rref.  The loop of k_rref (blz_kernels.hip) on u64 rows with a 64-bit stride: lanes hold one column each, a workgroup
 * keeps its echelon in LDS, reduces a tile of rows against it in parallel and inserts what is left, and a workgroup that
 * reaches rank n raises a flag every workgroup reads once per tile -- a block of full rank is not read whole.
 */
#include "blz_devsmall.h"
#include "blz_devhelp.h"

#include <algorithm>

namespace {

constexpr int BLOCK = 256;
constexpr int MAXN = 64;

MODP_DEV u64 submod(u64 a, u64 b, u64 p) { return a >= b ? a - b : a + (p - b); }

/* invmod(), sequential/lanczos_modp.c:318-336 (extended Euclid; |t| <= p < 2^62 throughout) */
MODP_DEV u64 inv_euclid(u64 a, u64 p)
{
	long long t = 0, nt = 1, r = (long long)p, nr = (long long)(a % p);
	while (nr != 0) {
		const long long q = r / nr;
		long long s = nt;
		nt = t - q * nt;
		t = s;
		s = nr;
		nr = r - q * nr;
		r = s;
	}
	if (t < 0)
		t += (long long)p;
	return (u64)t;
}

/* x^2 and x * y mod 2^61 - 1 for RESIDUES below 2^61 from three / four 32 x 32 products (sqrmod61 and mulmod61_res of
 * blz_kernels.hip): with x = x1 2^32 + x0, x1 < 2^29, and 2^61 = 1 the top product is 8 x1 y1, the middle ones fold at bit 29
 * (28 for the doubled one of a square) and the low one folds once.  About half the instructions of the 128-bit product. */
MODP_DEV u64 sqr61(u64 x)
{
	const u64 P = (1ull << 61) - 1;
	const u32 x0 = (u32)x, x1 = (u32)(x >> 32);
	const u64 lo = (u64)x0 * x0, mid = (u64)x0 * x1, hi = (u64)x1 * x1;
	const u64 t = (lo & P) + (lo >> 61) + (mid >> 28) + ((mid & ((1ull << 28) - 1)) << 33) + (hi << 3);	/* < 4 * 2^61 */
	const u64 r = (t & P) + (t >> 61);
	return r >= P ? r - P : r;
}

MODP_DEV u64 mul61(u64 x, u64 y)
{
	const u64 P = (1ull << 61) - 1;
	const u32 x0 = (u32)x, x1 = (u32)(x >> 32), y0 = (u32)y, y1 = (u32)(y >> 32);
	const u64 lo = (u64)x0 * y0, mid = (u64)x0 * y1 + (u64)x1 * y0, hi = (u64)x1 * y1;	/* mid < 2^62 */
	const u64 t = (lo & P) + (lo >> 61) + (mid >> 29) + ((mid & ((1ull << 29) - 1)) << 32) + (hi << 3);	/* < 4 * 2^61 */
	const u64 r = (t & P) + (t >> 61);
	return r >= P ? r - P : r;
}

/* product of two residues with the lean form where the prime has one */
template <int MERS>
MODP_DEV u64 mulres(u64 x, u64 y, const ModP &m)
{
	if (MERS == 61)
		return mul61(x, y);
	return mulmod<MERS>(x, y, m);
}

/* a^(p-2) for the two Mersenne primes: the inverse mod a prime is unique, so the word is the Euclid's, and a chain of
 * Mersenne products has no 64-bit division in it.  p - 2 = 2^b - 3 is b - 2 ones, a zero and a one. */
template <int MERS>
MODP_DEV u64 sqn(u64 x, int k, const ModP &m)	/* x^(2^k) */
{
	for (int i = 0; i < k; i++)
		x = MERS == 61 ? sqr61(x) : mulmod<MERS>(x, x, m);
	return x;
}

template <int MERS>
MODP_DEV u64 inv_fermat(u64 a, const ModP &m)
{
	const u64 x1 = a;
	const u64 x2 = mulres<MERS>(sqn<MERS>(x1, 1, m), x1, m);
	const u64 x3 = mulres<MERS>(sqn<MERS>(x2, 1, m), x1, m);
	const u64 x6 = mulres<MERS>(sqn<MERS>(x3, 3, m), x3, m);
	const u64 x12 = mulres<MERS>(sqn<MERS>(x6, 6, m), x6, m);
	const u64 x24 = mulres<MERS>(sqn<MERS>(x12, 12, m), x12, m);
	if (MERS == 31) {	/* exponents 2^k - 1 along 1, 2, 3, 6, 12, 24, 27, 29 */
		const u64 x27 = mulres<MERS>(sqn<MERS>(x24, 3, m), x3, m);
		const u64 x29 = mulres<MERS>(sqn<MERS>(x27, 2, m), x2, m);
		return mulres<MERS>(sqn<MERS>(x29, 2, m), x1, m);
	}
	/* 1, 2, 3, 6, 12, 24, 48, 54, 57, 59 */
	const u64 x48 = mulres<MERS>(sqn<MERS>(x24, 24, m), x24, m);
	const u64 x54 = mulres<MERS>(sqn<MERS>(x48, 6, m), x6, m);
	const u64 x57 = mulres<MERS>(sqn<MERS>(x54, 3, m), x3, m);
	const u64 x59 = mulres<MERS>(sqn<MERS>(x57, 2, m), x2, m);
	return mulres<MERS>(sqn<MERS>(x59, 2, m), x1, m);
}

template <int MERS>
MODP_DEV u64 inv_any(u64 a, const ModP &m)
{
	if (MERS != 0)
		return inv_fermat<MERS>(a, m);
	return inv_euclid(a, m.p);
}

/* s * x + f * y mod p for residues: below 2 p^2, one reduction */
template <int MERS>
MODP_DEV u64 axpy(u64 s, u64 x, u64 f, u64 y, const ModP &m)
{
	Acc acc;
	acc_zero(acc);
	acc_mac64(acc, s, x);
	acc_mac64(acc, f, y);
	return acc_reduce<MERS>(acc, m);
}

/*
 * One fraction-free Gauss-Jordan sweep with the pivot rule of sequential/lanczos_modp.c:351-381 / :393-436: for column j the
 * first non-zero entry in rows j .. n-1; a column without one is skipped; the pivot row goes to row j; column j is
 * eliminated from every other row:  row_i <- s_j * row_i - row_i[j] * row_j,  s_i <- s_i * s_j  (s_j = the pivot).  Wm and S
 * may be nullptr (the reference's phase 1 wants the pivot columns only).  Returns the pivot count and the pivot columns as a
 * mask (by value: a local whose address is taken would live in scratch); both are the same in every thread.  Ends with a barrier.
 */
struct Pivots {
	int count;
	u64 mask;
};

template <int MERS>
__device__ Pivots sweep(u64 *A, u64 *Wm, u64 *S, int n, int lg, const ModP &m)
{
	const int t = threadIdx.x, lane = t & 63, li = t >> lg, k = t & ((1 << lg) - 1), RP = (int)blockDim.x >> lg;
	int found = 0;
	u64 bits = 0;
	for (int j = 0; j < n; j++) {
		__syncthreads();	/* the column before this one has been eliminated */
		const u64 probe = (lane < n && lane >= j) ? A[lane * n + j] : 0;
		const unsigned long long cand = __ballot(probe != 0);	/* the same in every wavefront */
		if (cand == 0)
			continue;
		const int piv = __ffsll(cand) - 1;
		bits |= 1ull << j;
		found++;
		if (piv != j) {
			__syncthreads();	/* every wavefront has probed column j */
			if (t < n) {
				u64 x = A[piv * n + t];
				A[piv * n + t] = A[j * n + t];
				A[j * n + t] = x;
				if (Wm) {
					x = Wm[piv * n + t];
					Wm[piv * n + t] = Wm[j * n + t];
					Wm[j * n + t] = x;
				}
			}
			if (S && t == 0)
				S[piv] = S[j];
			__syncthreads();
		}
		const u64 pv = A[j * n + j];
		if (S && t == 0)
			S[j] = pv;
		for (int ib = 0; ib < n; ib += RP) {
			const int i = ib + li;
			if (i >= n || i == j || k >= n)
				continue;
			const u64 f = A[i * n + j];	/* read by the whole row, written by nobody: column j is dead from here on */
			if (f == 0)
				continue;
			const u64 neg = m.p - f;
			if (k > j)
				A[i * n + k] = axpy<MERS>(pv, A[i * n + k], neg, A[j * n + k], m);
			if (Wm)
				Wm[i * n + k] = axpy<MERS>(pv, Wm[i * n + k], neg, Wm[j * n + k], m);
			if (S && k == 0)
				S[i] = mulmod<MERS>(S[i], pv, m);
		}
	}
	__syncthreads();
	return Pivots{ found, bits };
}

/* LDS of k_dev_chain in words: the matrices, then S and Pre (MAXN words each) */
inline size_t chain_lds_words(int n, bool coef)
{
	return (size_t)(coef ? 4 : 3) * n * n + 2 * MAXN;
}

template <int MERS>
__global__ void __launch_bounds__(1024)
k_dev_chain(const u64 *__restrict__ vtav, const u64 *__restrict__ vtaav, u64 *__restrict__ winv, u64 *__restrict__ dvec,
	    u64 *__restrict__ coef, u64 *__restrict__ npiv_out, int n, int lg, ModP m)
{
	extern __shared__ __attribute__((aligned(16))) u64 lds[];
	const int nn = n * n, t = threadIdx.x, T = (int)blockDim.x;
	u64 *A = lds, *Wm = A + nn, *V1 = Wm + nn, *V2 = V1 + nn;	/* V2 only with coef */
	u64 *S = lds + (size_t)(coef ? 4 : 3) * nn, *Pre = S + MAXN;
	for (int e = t; e < nn; e += T) {
		const u64 x = vtav[e];
		A[e] = x;
		V1[e] = x;
		Wm[e] = (e / n == e % n) ? 1 : 0;
		if (coef)
			V2[e] = vtaav[e];
	}
	if (t < n)
		S[t] = 1;
	/* one sweep on the unmasked matrix while every column pivots (the mask of :384-388 is then all ones); the reference's
	 * two sweeps otherwise */
	Pivots pv = sweep<MERS>(A, Wm, S, n, lg, m);
	if (pv.count != n) {
		for (int e = t; e < nn; e += T)
			A[e] = V1[e];
		const u64 sel = sweep<MERS>(A, nullptr, nullptr, n, lg, m).mask;	/* phase 1, :349-382: which columns */
		for (int e = t; e < nn; e += T) {			/* :384-388 */
			const int i = e / n, j = e % n;
			const bool both = ((sel >> i) & 1) && ((sel >> j) & 1);
			A[e] = both ? V1[e] : 0;
			Wm[e] = (i == j && ((sel >> i) & 1)) ? 1 : 0;
		}
		if (t < n)
			S[t] = 1;
		pv = sweep<MERS>(A, Wm, S, n, lg, m);	/* phase 2, :389-436 */
	}
	const int npiv = pv.count;
	const u64 dbits = pv.mask;
	/* 1 / s_i for every row from one inversion: Pre[i] = s_0 .. s_i, then walk back */
	if (t == 0) {
		u64 run = 1;
		for (int i = 0; i < n; i++) {
			run = mulmod<MERS>(run, S[i], m);
			Pre[i] = run;
		}
		u64 inv = inv_any<MERS>(run, m);
		for (int i = n - 1; i >= 0; i--) {
			const u64 si = S[i];
			S[i] = i ? mulmod<MERS>(inv, Pre[i - 1], m) : inv;
			inv = mulmod<MERS>(inv, si, m);
		}
	}
	__syncthreads();
	u64 *wout = coef ? coef + (size_t)4 * nn : winv;	/* panel P_V is W */
	for (int e = t; e < nn; e += T) {
		const u64 w = mulmod<MERS>(Wm[e], S[e / n], m);
		Wm[e] = w;
		wout[e] = w;
	}
	if (t == 0 && npiv_out)
		*npiv_out = (u64)npiv;
	if (!coef) {
		if (t < n)
			dvec[t] = (dbits >> t) & 1;
		return;
	}
	__syncthreads();
	/* D | (I - D) - W * S | -vtav * D | I - D | W, S = vtaav's column where d is set and vtav's where it is not (:460-475) */
	for (int e = t; e < nn; e += T) {
		const int i = e / n, j = e % n;
		const bool dj = (dbits >> j) & 1;
		const u64 *sp = dj ? V2 : V1;
		Acc acc;
		acc_zero(acc);
		u32 cnt = 0;
		for (int k = 0; k < n; k++) {
			acc_mac64(acc, Wm[i * n + k], sp[k * n + j]);
			if (++cnt == m.chunk) {
				cnt = 0;
				acc_set(acc, acc_reduce<MERS>(acc, m));
			}
		}
		const u64 r = acc_reduce<MERS>(acc, m);
		const u64 keep = (i == j && !dj) ? 1 : 0;	/* I - D */
		const u64 x = V1[e];
		coef[e] = (i == j && dj) ? 1 : 0;
		coef[(size_t)nn + e] = submod(keep, r, m.p);
		coef[(size_t)2 * nn + e] = (dj && x) ? m.p - x : 0;
		coef[(size_t)3 * nn + e] = keep;
	}
}

/* ---------------------------------------------------------------------------------------------------------------- echelon */

#define DEVRREF_U 8

/* k_rref of blz_kernels.hip on u64 rows with a 64-bit row stride.  MERGE: one workgroup over the stack (*rows_dev rows of
 * stride n), which writes E sorted by pivot column, info (int64) and the null basis. */
template <int MERS, bool MERGE>
__global__ void __launch_bounds__(BLOCK)
k_dev_rref(const u64 *__restrict__ X, long long rows_arg, const int *rows_dev, long long ld, int n, int G, ModP m, int *ctl,
	   u64 *__restrict__ out, u64 *__restrict__ zout, long long *__restrict__ info)
{
	__shared__ u64 E[MAXN * MAXN];
	__shared__ u64 s_row[MAXN];
	__shared__ int piv[MAXN], order[MAXN], freecol[MAXN];
	__shared__ int s_rank, s_stop, s_base, s_first, s_q;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int col = lane & (G - 1), sub = lane / G, rpw = 64 / G;
	const int TR = (BLOCK / 64) * DEVRREF_U * rpw;
	const long long rows = rows_dev ? (long long)*rows_dev : rows_arg;
	if (tid == 0)
		s_rank = 0;
	const long long ntiles = (rows + TR - 1) / TR;
	for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
		if (tid == 0)
			s_stop = s_rank == n || (!MERGE && __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
		__syncthreads();
		if (s_stop)
			break;
		const int r = s_rank;
		const long long base = tile * TR;
		u64 y[DEVRREF_U];
#pragma unroll
		for (int u = 0; u < DEVRREF_U; u++) {
			const long long row = base + (long long)((wave * DEVRREF_U + u) * rpw + sub);
			y[u] = (row < rows && col < n) ? X[row * ld + col] : 0;
		}
		if (r > 0) {
			Acc acc[DEVRREF_U];
#pragma unroll
			for (int u = 0; u < DEVRREF_U; u++)
				acc_set(acc[u], y[u]);
			u32 cnt = 0;
			for (int j = 0; j < r; j++) {
				const u64 e = E[j * MAXN + col];
				const u64 ne = (col < n && e) ? m.p - e : 0;	/* - E_j[col] */
				const int src = sub * G + piv[j];
#pragma unroll
				for (int u = 0; u < DEVRREF_U; u++)
					acc_mac64(acc[u], shfl64(y[u], src), ne);
				if (++cnt == m.chunk) {
#pragma unroll
					for (int u = 0; u < DEVRREF_U; u++)
						acc_set(acc[u], acc_reduce<MERS>(acc[u], m));
					cnt = 0;
				}
			}
#pragma unroll
			for (int u = 0; u < DEVRREF_U; u++)
				y[u] = acc_reduce<MERS>(acc[u], m);
		}
		/* insert the tile's first non-zero remainder, reduce the tile by it, repeat: at most n times per workgroup */
		for (;;) {
			int first = 0x7fffffff;
#pragma unroll
			for (int u = DEVRREF_U - 1; u >= 0; u--)
				if (y[u] != 0)
					first = (wave * DEVRREF_U + u) * rpw + sub;
			if (tid == 0)
				s_first = 0x7fffffff;
			__syncthreads();
			if (first != 0x7fffffff)
				atomicMin(&s_first, first);
			__syncthreads();
			const int tf = s_first;
			if (tf == 0x7fffffff || s_rank == n)
				break;
#pragma unroll
			for (int u = 0; u < DEVRREF_U; u++)
				if ((wave * DEVRREF_U + u) * rpw + sub == tf && col < n)
					s_row[col] = y[u];
			__syncthreads();
			if (wave == 0) {
				const int c = lane;
				const int rr = s_rank;
				const u64 x = c < n ? s_row[c] : 0;
				const int q = __ffsll((long long)__ballot(x != 0)) - 1;
				const u64 row = mulmod<MERS>(x, inv_any<MERS>(shfl64(x, q), m), m);	/* row[q] = 1 */
				for (int j = 0; j < rr; j++) {
					const u64 f = E[j * MAXN + q];	/* read by every lane before lane q clears it */
					if (f && c < n)
						E[j * MAXN + c] = submod(E[j * MAXN + c], mulmod<MERS>(f, row, m), m.p);
				}
				E[rr * MAXN + c] = c < n ? row : 0;
				if (c < n)
					s_row[c] = row;
				if (c == 0) {
					piv[rr] = q;
					s_q = q;
					s_rank = rr + 1;
				}
			}
			__syncthreads();
			/* y <- y - y[q] * row: zero at q, and still zero at the older pivots (row is zero there) */
			const int src = sub * G + s_q;
			const u64 nrow = col < n ? s_row[col] : 0;
#pragma unroll
			for (int u = 0; u < DEVRREF_U; u++) {
				const u64 f = shfl64(y[u], src);
				y[u] = submod(y[u], mulmod<MERS>(f, nrow, m), m.p);
			}
			if (!MERGE && tid == 0 && s_rank == n)
				__hip_atomic_store(&ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	__syncthreads();
	const int r = s_rank;
	if (!MERGE) {
		if (tid == 0)
			s_base = r ? atomicAdd(&ctl[1], r) : 0;
		__syncthreads();
		for (int k = tid; k < r * n; k += BLOCK)
			out[(size_t)(s_base + k / n) * n + k % n] = E[(k / n) * MAXN + k % n];
		return;
	}
	/* order[pos] = the echelon row whose pivot column is the pos-th smallest; the pivot columns as a mask */
	if (tid < r) {
		int pos = 0;
		for (int j = 0; j < r; j++)
			pos += piv[j] < piv[tid];
		order[pos] = tid;
	}
	__syncthreads();
	u64 pmask = 0;
	for (int j = 0; j < r; j++)
		pmask |= 1ull << piv[j];
	if (tid < n && !((pmask >> tid) & 1))	/* the free columns, ascending */
		freecol[__popcll(~pmask & ((1ull << tid) - 1))] = tid;
	__syncthreads();
	/* rows sorted by pivot column; rows r .. n-1 zero */
	for (int k = tid; k < n * n; k += BLOCK) {
		const int i = k / n, cc = k % n;
		out[k] = i < r ? E[order[i] * MAXN + cc] : 0;
		if (zout) {
			/* column cc of the null basis belongs to free column f: 1 at f, -e[i'][f] at the pivot of row i' */
			u64 zv = 0;
			if (cc < n - r) {
				const int f = freecol[cc];
				if (i == f) {
					zv = 1;
				} else if ((pmask >> i) & 1) {
					const u64 ev = E[order[__popcll(pmask & ((1ull << i) - 1))] * MAXN + f];
					zv = ev ? m.p - ev : 0;
				}
			}
			zout[k] = zv;
		}
	}
	if (tid < n)
		info[1 + tid] = tid < r ? (long long)piv[order[tid]] : -1;
	if (tid == 0)
		info[0] = r;
}

inline int group_of(int n)
{
	int G = 1;
	while (G < n)
		G <<= 1;
	return G;
}

int partial_blocks(const KernelCfg &c, long long rows, int n)
{
	const int TR = (BLOCK / 64) * DEVRREF_U * (64 / group_of(n));
	const long long tiles = (rows + TR - 1) / TR;
	const long long b = std::min<long long>(tiles, (long long)c.num_cu * 2);
	return (int)std::max<long long>(b, 1);
}

template <int MERS>
hipError_t chain_go(unsigned threads, size_t lds, hipStream_t s, const u64 *vtav, const u64 *vtaav, u64 *winv, u64 *d, u64 *coef,
		    u64 *npiv, int n, int lg, const ModP &m)
{
	const hipError_t e = dev_lds_limit<&k_dev_chain<MERS>>(lds, chain_lds_words(MAXN, true) * sizeof(u64));
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL((k_dev_chain<MERS>), dim3(1), dim3(threads), lds, s, vtav, vtaav, winv, d, coef, npiv, n, lg, m);
	return hipGetLastError();
}

template <int MERS>
void rref_go(int blocks, hipStream_t s, long long rows, const u64 *x, long long ldx, int n, const ModP &m, u64 *stack, int *ctl, u64 *e,
	     u64 *z, long long *info)
{
	const int G = group_of(n);
	hipLaunchKernelGGL((k_dev_rref<MERS, false>), dim3((unsigned)blocks), dim3(BLOCK), 0, s, x, rows, nullptr, ldx, n, G, m, ctl, stack,
			   nullptr, nullptr);
	hipLaunchKernelGGL((k_dev_rref<MERS, true>), dim3(1), dim3(BLOCK), 0, s, stack, 0ll, ctl + 1, (long long)n, n, G, m, nullptr, e, z,
			   info);
}

}  // namespace

hipError_t launch_dev_chain(const KernelCfg &c, int n, const u64 *vtav, const u64 *vtaav, u64 *winv, u64 *d, u64 *coef, u64 *npiv,
			    hipStream_t s)
{
	if (n < 1 || n > MAXN || !vtav || (coef ? !vtaav : (!winv || !d)))
		return hipErrorInvalidValue;
	const int lg = log2_ceil(n);
	const unsigned threads = (unsigned)std::min(1024, std::max(64, 1 << (2 * lg)));
	const size_t lds = chain_lds_words(n, coef != nullptr) * sizeof(u64);
	if (c.mers == 61)
		return chain_go<61>(threads, lds, s, vtav, vtaav, winv, d, coef, npiv, n, lg, c.m);
	if (c.mers == 31)
		return chain_go<31>(threads, lds, s, vtav, vtaav, winv, d, coef, npiv, n, lg, c.m);
	return chain_go<0>(threads, lds, s, vtav, vtaav, winv, d, coef, npiv, n, lg, c.m);
}

long long dev_rref_stack_rows(const KernelCfg &c, int n)
{
	return (long long)c.num_cu * 2 * n;
}

hipError_t launch_dev_rref(const KernelCfg &c, int n, long long rows, const u64 *x, long long ldx, u64 *stack, int *ctl, u64 *e,
			   u64 *z, long long *info, hipStream_t s)
{
	if (n < 1 || n > MAXN || rows < 0 || ldx < n || !stack || !ctl || !e || !info)
		return hipErrorInvalidValue;
	hipError_t err = hipMemsetAsync(ctl, 0, 2 * sizeof(int), s);
	if (err != hipSuccess)
		return err;
	const int b = partial_blocks(c, rows, n);
	if (c.mers == 61)
		rref_go<61>(b, s, rows, x, ldx, n, c.m, stack, ctl, e, z, info);
	else if (c.mers == 31)
		rref_go<31>(b, s, rows, x, ldx, n, c.m, stack, ctl, e, z, info);
	else
		rref_go<0>(b, s, rows, x, ldx, n, c.m, stack, ctl, e, z, info);
	return hipGetLastError();
}
