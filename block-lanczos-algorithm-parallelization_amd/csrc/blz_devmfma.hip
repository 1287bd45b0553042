/*
 * blz_devmfma.hip -- the device block algebra on the matrix cores: blz_dot_device, blz_dot_pair_device, blz_combine_device and
 * blz_combine_pair_device at p = 2^61 - 1, n = 8 or 16, on a caller's strided u64 rows.  Exact integer
 * contractions of base-256 digits on v_mfma_i32_16x16x64_i8; the words written are the ones the vector-ALU kernels of
 * blz_devalg.hip write.  Which form a call takes is decided in blz_devmfma_plan.h.
 *
 * k_dm_combine: Z = sum_t X_t * A_t, the scheme of k_ortho_mfma (header comment of blz_dense_mfma.hip) without its non-product
 * term and with the rows at the caller's stride.
 *   - the bytes of a row of X_0 | X_1 | ... are the A operand after XOR 0x80 (u -> u - 128): K' = (term, word k, byte a),
 *     8 n nterms of them, 64 per MFMA.  Lane (m, h) of a 16-row tile takes bytes 16 h .. 16 h + 15 of each 64-byte part of row m
 *     with one 16-byte load (the base is 16-byte aligned and the stride even, or the call is not here).
 *   - byte a of word k weighs 2^(8a): k_dm_prep rewrites every coefficient as rot61(a_t[k][j], 8 a), one 61-bit multiplier per
 *     K', in 8 SIGNED base-256 digits; digit position s of all of them is the B operand B_s, in fragment order in the image.
 *   - acc_s = sum over K' of (u - 128) B_s is one chain of MFMAs that starts at 128 * (column sum of B_s) + DM_START: the digit
 *     sum S_s = DM_START + sum u d lies in [0, DM_SUM_MAX] (blz_devmfma_plan.h), below 2^25.
 *   - sum_s S_s 2^(8s): one v_mad_u64_u32 per digit sum into two 64-bit sums (s < 4, s >= 4), one fold mod 2^61 - 1, and the
 *     starts' total is subtracted mod p.
 * n = 16: tile columns = the 16 columns of Z; the pair runs two chains (two images) over the same A fragments.  n = 8: the
 * pair puts Z0 | Z1 in the 16 tile columns (one chain); the single form leaves columns 8..15 zero.
 * In place: a wavefront loads its tile's rows of every term, multiplies, and only then stores; no other wavefront touches
 * those rows.
 *
 * k_dm_dot: C = X^T Y, the scheme of k_block_dot_mfma with the ROWS as the K dimension: a lane holds 16 rows of one column,
 * byte a of each gathered into a fragment; both operands are biased, which the algebra turns into column sums:
 *     sum_r X[r,i] Y[r,j] = sum_s 2^(8s) sum_{a+b=s} C_ab[i][j] + 128 W (colsum_X[i] + colsum_Y[j]) - 16384 R W^2
 * (W = sum_a 2^(8a), R = rows processed, rows past the end being zero words).  The 15 int32 accumulators of a product start at
 * 2^30 and are folded every DM_DOT_FOLD_TILES tiles of 64 rows, before they can leave [2^29, 3 * 2^29].
 * n = 16: operands X_p and Y, one product per left block.  n = 8, one left block: ONE operand [X | Y], whose product with
 * itself holds X^T Y in its upper right 8 x 8; n = 8, two: [X0 | X1] against [Y | Y], X0^T Y above X1^T Y in columns 0..7.
 * Every workgroup writes one partial row; launch_dev_dot_finalize (blz_devalg.h) adds them mod p.
 */
#include "blz_devmfma.h"
#include "blz_devhelp.h"
#include "ortho_img.h"

#include <type_traits>

namespace {

constexpr u64 P61 = (1ull << 61) - 1;

/* ------------------------------------------------------------------------------------------------ recombination */

struct DmCombineArgs {
	const u64 *x[DM_MAX_TERMS];
	long long ldx[DM_MAX_TERMS];
	const u64 *a0[DM_MAX_TERMS], *a1[DM_MAX_TERMS];	/* NULL: a zero panel */
	u64 *z0, *z1;
	long long ldz0, ldz1;
};

/* coefficient of K' word kk (term kk / NT, word kk % NT of its row) and tile column col in image `set` */
template <int NT>
MODP_DEV u64 dm_coef(const DmCombineArgs &g, int set, int kk, int col)
{
	const int t = kk / NT, k = kk % NT;
	const u64 *a;
	int c;
	if (NT == 16) {
		a = set == 0 ? g.a0[t] : g.a1[t];
		c = col;
	} else {
		a = col < 8 ? g.a0[t] : g.a1[t];
		c = col & 7;
	}
	return a ? a[k * NT + c] : 0;
}

/* the image of one launch: sets * ksteps * 8 KB of digits in fragment order -- [set][K step][digit position][lane][16 bytes],
 * lane = 16 (K' / 16 within the step) + column -- then the accumulator starts, one wavefront per entry with its K' over the
 * lanes (the structure of k_ortho_mfma_prep) */
template <int NT>
__global__ void __launch_bounds__(256)
k_dm_prep(DmCombineArgs g, int sets, int ksteps, unsigned char *__restrict__ img)
{
	const int t = threadIdx.x;
	signed char *B = (signed char *)img;
	const int bbytes = (int)dm_image_b_bytes(sets, ksteps);
	for (int idx = blockIdx.x * 256 + t; idx < bbytes; idx += gridDim.x * 256) {
		const int j = idx & 15, ln = (idx >> 4) & 63, dg = (idx >> 10) & 7, q = idx >> 13;
		const int set = q / ksteps, ks = q % ksteps;
		const int E = 64 * ks + 16 * (ln >> 4) + j;
		/* idx == dm_image_frag_at(ksteps, set, ks, dg, ln) + j */
		B[idx] = (signed char)signed_digit(rot61(dm_coef<NT>(g, set, E >> 3, ln & 15), 8 * (E & 7)), dg);
	}
	const int ne = sets * DM_ND * 16;
	for (int e = (blockIdx.x * 256 + t) >> 6; e < ne; e += (int)gridDim.x * 4) {
		const int col = e & 15, dg = (e >> 4) & 7, set = e >> 7;
		int sum = 0;
		for (int kp = t & 63; kp < ksteps * 64; kp += 64)
			sum += signed_digit(rot61(dm_coef<NT>(g, set, kp >> 3, col), 8 * (kp & 7)), dg);
		for (int off = 32; off; off >>= 1)
			sum += __shfl_xor(sum, off, 64);
		if ((t & 63) == 0)
			*(int *)(img + dm_image_init_at(sets, ksteps, set, dg, col)) = 128 * sum + DM_START;
	}
}

/* the DM_START added to each of the 8 digit sums, with their weights 2^(8 s): minus their sum mod 2^61 - 1, added at the end */
constexpr u64 dm_bias_correction(void)
{
	unsigned __int128 bias = 0;
	for (int dg = 0; dg < DM_ND; dg++)
		bias += (unsigned __int128)DM_START << (8 * dg);
	const u64 r = (u64)(bias % P61);
	return r ? P61 - r : 0;
}

/* workgroups of up to 1024 threads (128 registers); the pair at n = 16, two chains, needs more than 128 at three and four terms
 * and runs at most 512 (blz_devmfma_plan.h) */
template <int NT, int NTERMS, int SETS>
__global__ void __launch_bounds__((SETS == 2 ? 512 : 1024))
k_dm_combine(DmCombineArgs g, int pair, long long rows, const unsigned char *__restrict__ img)
{
	/* (no __restrict__ on the blocks: an output may be one of the terms) */
	constexpr int NLD = NT / 8, KS = NLD * NTERMS;		/* 64-byte parts of a row; K steps */
	constexpr int IMG_BYTES = (SETS * KS * DM_ND * 64 + SETS * DM_ND * 4) * 16;	/* = dm_image_bytes(SETS, KS) */
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	{
		const uint4 *src = (const uint4 *)img;
		uint4 *dst = (uint4 *)lds;
		for (int i = threadIdx.x; i < IMG_BYTES / 16; i += (int)blockDim.x)
			dst[i] = src[i];
	}
	__syncthreads();
	constexpr u64 fconst = dm_bias_correction();
	u32 one;
	asm volatile("s_mov_b32 %0, 1" : "=s"(one));	/* 1, opaque to the optimiser (see dm_mad_u64) */
	const int lane = threadIdx.x & 63, m = lane & 15, h = lane >> 4, col = m;
	const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
	const long long ntiles = (rows + 15) >> 4;
	for (long long tile = wave; tile < ntiles; tile += nwaves) {
		const long long r0 = tile << 4;
		/* A fragments: row m of every term, 16 bytes per K step, biased to signed.  Rows past the end: any valid address
		 * (the tile's own last row), their results are not stored */
		long long rr = r0 + m;
		rr = rr < rows ? rr : rows - 1;
		dm_v4i A[KS];
#pragma unroll
		for (int t = 0; t < NTERMS; t++) {
			const unsigned char *row = (const unsigned char *)(g.x[t] + rr * g.ldx[t]);
#pragma unroll
			for (int q = 0; q < NLD; q++)
				A[t * NLD + q] = *(const dm_v4i *)(row + 64 * q + 16 * h);
		}
#pragma unroll
		for (int q = 0; q < KS; q++)
			A[q] ^= (dm_v4i){ (int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080 };
		u64 L[SETS][4], H[SETS][4];
#pragma unroll
		for (int st = 0; st < SETS; st++)
#pragma unroll
			for (int reg = 0; reg < 4; reg++)
				L[st][reg] = H[st][reg] = 0;
#pragma unroll
		for (int s = 0; s < DM_ND; s++) {
			const u32 mul = one << (s < 4 ? 8 * s : 8 * (s - 4));
#pragma unroll
			for (int st = 0; st < SETS; st++) {
				const int i0 = *(const int *)(lds + dm_image_init_at(SETS, KS, st, s, col));
				dm_v4i acc = { i0, i0, i0, i0 };
#pragma unroll
				for (int ks = 0; ks < KS; ks++)
					acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ks], *(const dm_v4i *)(lds + dm_image_frag_at(KS, st, ks, s, lane)),
										    acc, 0, 0, 0);
#pragma unroll
				for (int reg = 0; reg < 4; reg++) {
					if (s < 4)
						dm_mad_u64(L[st][reg], (u32)acc[reg], mul);
					else
						dm_mad_u64(H[st][reg], (u32)acc[reg], mul);
				}
			}
			/* keep the digit sums sequential: without this the compiler hoists all the fragment reads (and spills) */
			asm volatile("" ::: "memory");
		}
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const long long ro = r0 + 4 * h + reg;
			if (ro >= rows)
				continue;
			const u64 x = addmod(dm_fold61(L[0][reg], H[0][reg]), fconst, P61);
			if (NT == 16) {
				g.z0[ro * g.ldz0 + col] = x;
				if (SETS == 2)
					g.z1[ro * g.ldz1 + col] = addmod(dm_fold61(L[SETS - 1][reg], H[SETS - 1][reg]), fconst, P61);
			} else if (col < 8) {
				g.z0[ro * g.ldz0 + col] = x;
			} else if (pair) {
				g.z1[ro * g.ldz1 + (col - 8)] = x;
			}
		}
	}
}

/* (the image of an instantiation has one size: its LDS is the most it can ask for) */
template <int NT, int NTERMS, int SETS>
hipError_t combine_go(const dm_plan &pl, const DmCombineArgs &g, int pair, long long rows, const unsigned char *img, hipStream_t s)
{
	const hipError_t e = dev_lds_limit<&k_dm_combine<NT, NTERMS, SETS>>((size_t)pl.lds_bytes,
									     (size_t)dm_image_bytes(SETS, dm_combine_ksteps(NT, NTERMS)));
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL((k_dm_combine<NT, NTERMS, SETS>), dim3((unsigned)pl.blocks), dim3((unsigned)pl.threads), (size_t)pl.lds_bytes, s,
			   g, pair, rows, img);
	return hipGetLastError();
}

template <int NT, int SETS>
hipError_t combine_terms(int nterms, const dm_plan &pl, const DmCombineArgs &g, int pair, long long rows, const unsigned char *img,
			 hipStream_t s)
{
	switch (nterms) {
	case 1: return combine_go<NT, 1, SETS>(pl, g, pair, rows, img, s);
	case 2: return combine_go<NT, 2, SETS>(pl, g, pair, rows, img, s);
	case 3: return combine_go<NT, 3, SETS>(pl, g, pair, rows, img, s);
	default: return combine_go<NT, 4, SETS>(pl, g, pair, rows, img, s);
	}
}

/* ------------------------------------------------------------------------------------------------ inner products */

MODP_DEV u64 dm_shfl64(u64 x, int src)
{
	const u32 lo = (u32)__shfl((int)(u32)x, src, 64), hi = (u32)__shfl((int)(u32)(x >> 32), src, 64);
	return ((u64)hi << 32) | lo;
}

/* 16 rows of one column (rows past the end: zero words) and their sum, < 2^62 and congruent mod p */
MODP_DEV u64 dm_load16(u64 *w, const u64 *b, long long ld, int c, long long r0, long long rows, bool wanted)
{
#pragma unroll
	for (int q = 0; q < 16; q++) {
		const long long r = r0 + q;
		w[q] = wanted && r < rows ? b[r * ld + c] : 0;
	}
	u64 t = 0;
#pragma unroll
	for (int q = 0; q < 16; q += 4)
		t = dm_fold_partial61(t + w[q] + w[q + 1] + w[q + 2] + w[q + 3]);	/* words < 2^61 */
	return t;
}

/* two wavefronts per SIMD: 256 registers (accumulators included).  The pair at n = 16 -- 30 accumulators of four registers, three
 * operands at the caller's strides (a 64-bit address per row) -- does not fit them without scratch: it runs one per SIMD */
template <int NT, int NX>
__global__ void __launch_bounds__(DM_DOT_THREADS, (NT == 16 && NX == 2 ? 1 : 2))
k_dm_dot(const u64 *__restrict__ x0, long long ldx0, const u64 *__restrict__ x1, long long ldx1, const u64 *__restrict__ y,
	 long long ldy, long long rows, int same01, int same0y, int same1y, u64 *__restrict__ partial)
{
	constexpr int NP = NT == 16 ? NX : 1, WAVES = DM_DOT_THREADS / 64, NN = NT * NT;
	constexpr bool SELF = NT == 8 && NX == 1;	/* one operand [X | Y] on both sides */
	__shared__ u64 red[WAVES][NP][4][64];
	__shared__ u64 csum[WAVES][3][64];
	__shared__ long long tiles_sh[WAVES];
	u32 one;
	asm volatile("s_mov_b32 %0, 1" : "=s"(one));
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, h = lane >> 4;
	const long long wave = (long long)blockIdx.x * WAVES + wv, nwaves = (long long)gridDim.x * WAVES;
	const long long ntiles = (rows + 63) >> 6;
	/* this lane's column of the right operand B and of the left operands A_p, and whether A_p's column IS B's (same block) */
	const u64 *pb = SELF && m < 8 ? x0 : y;
	const long long ldb = SELF && m < 8 ? ldx0 : ldy;
	const int cb = NT == 16 ? m : (m & 7);
	const u64 *pa[2] = { NT == 16 || m < 8 ? x0 : x1, x1 };
	const long long lda[2] = { NT == 16 || m < 8 ? ldx0 : ldx1, ldx1 };
	const bool isb[2] = { (NT == 16 || m < 8 ? same0y : same1y) != 0, same1y != 0 };
	dm_v4i acc[NP][15];
	u64 res[NP][4];
#pragma unroll
	for (int p_ = 0; p_ < NP; p_++) {
#pragma unroll
		for (int s = 0; s < 15; s++)
			acc[p_][s] = (dm_v4i){ 1 << 30, 1 << 30, 1 << 30, 1 << 30 };
#pragma unroll
		for (int reg = 0; reg < 4; reg++)
			res[p_][reg] = 0;
	}
	u64 csb = 0, csa[2] = { 0, 0 };		/* column sums (mod p, lazily folded) of this lane's column of B / A_p */
	long long nflush = 0, ntl = 0;
	int pending = 0;
	auto flush = [&]() {
#pragma unroll
		for (int p_ = 0; p_ < NP; p_++) {
#pragma unroll
			for (int reg = 0; reg < 4; reg++) {
				u64 L = 0, H = 0;
#pragma unroll
				for (int s = 0; s < 15; s++) {
					const int sh = dm_fold_shift(s);
					const u32 mul = one << (sh < 32 ? sh : sh - 32);
					if (sh < 32)
						dm_mad_u64(L, (u32)acc[p_][s][reg], mul);
					else
						dm_mad_u64(H, (u32)acc[p_][s][reg], mul);
				}
				/* L < 8 * 2^31 * 2^27 = 2^61, H likewise: fold H first so that dm_fold61's bounds hold */
				const u64 x = dm_fold61(L, 0), yy = dm_fold61(H, 0);
				const unsigned __int128 t = (unsigned __int128)yy << 32;	/* yy * 2^32 mod p */
				u64 z = ((u64)t & P61) + (u64)(t >> 61);
				z = (z & P61) + (z >> 61);
				z = z >= P61 ? z - P61 : z;
				res[p_][reg] = addmod(res[p_][reg], addmod(x, z, P61), P61);
			}
#pragma unroll
			for (int s = 0; s < 15; s++)
				acc[p_][s] = (dm_v4i){ 1 << 30, 1 << 30, 1 << 30, 1 << 30 };
		}
		nflush++;
		pending = 0;
	};
	for (long long tile = wave; tile < ntiles; tile += nwaves) {
		const long long r0 = (tile << 6) + 16 * h;
		u64 xv[16];
		dm_v4i fb[8];
		u64 tb;
		{
			u64 yv[16];
			tb = dm_load16(yv, pb, ldb, cb, r0, rows, true);
			dm_digit_fragments(yv, fb);
		}
		csb = dm_fold_partial61(csb + tb);
		if (SELF) {
#pragma unroll
			for (int a = 0; a < 8; a++) {
#pragma unroll
				for (int b = 0; b < 8; b++)
					acc[0][a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fb[a], fb[b], acc[0][a + b], 0, 0, 0);
			}
		} else {
#pragma unroll
			for (int p_ = 0; p_ < NP; p_++) {
				const bool same = isb[p_];
				/* one left block's words at a time: without this the compiler loads both up front (and spills) */
				asm volatile("" ::: "memory");
				/* a left block that is the right one, or the left one before it, is not read again */
				u64 ta = tb;
				if (p_ == 0 || !same01) {
					const u64 tl = dm_load16(xv, pa[p_], lda[p_], cb, r0, rows, !same);
					ta = same ? tb : tl;
					csa[p_] = dm_fold_partial61(csa[p_] + ta);
				} else {
					csa[p_] = csa[0];
				}
				auto left = [&](auto pr) {
					constexpr int PR_ = decltype(pr)::value;
					dm_v4i fv2[2];
					dm_digit_fragment_pair<PR_>(xv, fv2);
#pragma unroll
					for (int d = 0; d < 4; d++) {
						fv2[0][d] = same ? fb[2 * PR_][d] : fv2[0][d];
						fv2[1][d] = same ? fb[2 * PR_ + 1][d] : fv2[1][d];
					}
#pragma unroll
					for (int b = 0; b < 8; b++) {
						acc[p_][2 * PR_ + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv2[0], fb[b], acc[p_][2 * PR_ + b], 0, 0, 0);
						acc[p_][2 * PR_ + 1 + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv2[1], fb[b], acc[p_][2 * PR_ + 1 + b], 0, 0, 0);
					}
				};
				left(std::integral_constant<int, 0>{});
				left(std::integral_constant<int, 1>{});
				left(std::integral_constant<int, 2>{});
				left(std::integral_constant<int, 3>{});
			}
		}
		ntl++;
		if (++pending == DM_DOT_FOLD_TILES)
			flush();
	}
	if (pending)
		flush();
	/* the 2^30 every accumulator started from, per flush: nflush * 2^30 * sum_s 2^(8 s mod 61) */
	const ModP mp = { P61, 0, 61, 32 };
	u64 biasw = 0;
	for (int s = 0; s < 15; s++) {
		const unsigned __int128 t = (unsigned __int128)(1u << 30) << dm_fold_shift(s);
		biasw = addmod(biasw, (u64)(t % P61), P61);
	}
	const u64 bias_total = mulmod<61>(biasw, (u64)(nflush % (long long)P61), mp);
	/* per wave: residues in the accumulator layout (row i = 4 h + reg, column j = lane & 15) and the column sums */
#pragma unroll
	for (int p_ = 0; p_ < NP; p_++)
#pragma unroll
		for (int reg = 0; reg < 4; reg++)
			red[wv][p_][reg][lane] = addmod(res[p_][reg], bias_total ? P61 - bias_total : 0, P61);
	csum[wv][0][lane] = dm_fold61(csb, 0);
	csum[wv][1][lane] = dm_fold61(SELF ? csb : csa[0], 0);
	csum[wv][2][lane] = dm_fold61(NP == 2 ? csa[1] : 0, 0);
	if (lane == 0)
		tiles_sh[wv] = ntl;
	__syncthreads();
	if (wv != 0)
		return;
	/* wavefront 0: sum over the wavefronts, add the bias terms, write the partial row */
	long long tl = 0;
	for (int w = 0; w < WAVES; w++)
		tl += tiles_sh[w];
	/* W = sum_{a<8} 2^(8a) mod p, K1 = 128 W, K2 = 16384 W^2, 64 rows per tile */
	u64 W = 0;
	for (int a = 0; a < 8; a++)
		W = addmod(W, (u64)(((unsigned __int128)1 << (8 * a)) % P61), P61);
	const u64 K1 = mulmod<61>(W, 128, mp), K2 = mulmod<61>(mulmod<61>(W, W, mp), 16384, mp);
	const u64 k2r = mulmod<61>(K2, (u64)((tl * 64) % (long long)P61), mp);
	/* column sums over the 4 k-blocks (lanes m, m + 16, m + 32, m + 48) and the wavefronts: of column (lane & 15) */
	u64 colb = 0, cola[2] = { 0, 0 };
	for (int w = 0; w < WAVES; w++)
		for (int hh = 0; hh < 4; hh++) {
			colb = addmod(colb, csum[w][0][m + 16 * hh], P61);
			cola[0] = addmod(cola[0], csum[w][1][m + 16 * hh], P61);
			cola[1] = addmod(cola[1], csum[w][2][m + 16 * hh], P61);
		}
	u64 *out = partial + (size_t)blockIdx.x * NX * NN;
#pragma unroll
	for (int p_ = 0; p_ < NP; p_++) {
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const int i = 4 * h + reg, j = m;
			u64 x = 0;
			for (int w = 0; w < WAVES; w++)
				x = addmod(x, red[w][p_][reg][lane], P61);
			/* lane i (h = 0, m = i) holds the sums of column i: the row index of this output needs them from there */
			const u64 sx = dm_shfl64(cola[p_], i);
			x = addmod(x, mulmod<61>(K1, addmod(sx, colb, P61), mp), P61);
			x = addmod(x, k2r ? P61 - k2r : 0, P61);
			if (NT == 16) {
				out[p_ * NN + i * 16 + j] = x;
			} else if (NX == 1) {
				if (i < 8 && j >= 8)
					out[i * 8 + (j - 8)] = x;		/* X^T Y out of [X | Y]^T [X | Y] */
			} else if (j < 8) {
				out[(i >> 3) * NN + (i & 7) * 8 + j] = x;	/* X0^T Y above X1^T Y */
			}
		}
	}
}

}  // namespace

hipError_t launch_devmfma_dot(const dm_plan &pl, int n, long long rows, int nx, const u64 *x0, long long ldx0, const u64 *x1,
			      long long ldx1, const u64 *y, long long ldy, u64 *partial, int max_blocks, u64 *out, hipStream_t s)
{
	if (pl.form != 1 || (n != 8 && n != 16) || (nx != 1 && nx != 2) || rows < 1 || pl.blocks < 1 || pl.blocks > max_blocks ||
	    pl.threads != DM_DOT_THREADS)
		return hipErrorInvalidValue;
	if (nx == 1) {
		x1 = x0;
		ldx1 = ldx0;
	}
	const int same01 = x0 == x1 && ldx0 == ldx1, same0y = x0 == y && ldx0 == ldy, same1y = x1 == y && ldx1 == ldy;
	const dim3 grid((unsigned)pl.blocks), block(DM_DOT_THREADS);
	if (n == 16 && nx == 1)
		hipLaunchKernelGGL((k_dm_dot<16, 1>), grid, block, 0, s, x0, ldx0, x1, ldx1, y, ldy, rows, same01, same0y, same1y, partial);
	else if (n == 16)
		hipLaunchKernelGGL((k_dm_dot<16, 2>), grid, block, 0, s, x0, ldx0, x1, ldx1, y, ldy, rows, same01, same0y, same1y, partial);
	else if (nx == 1)
		hipLaunchKernelGGL((k_dm_dot<8, 1>), grid, block, 0, s, x0, ldx0, x1, ldx1, y, ldy, rows, same01, same0y, same1y, partial);
	else
		hipLaunchKernelGGL((k_dm_dot<8, 2>), grid, block, 0, s, x0, ldx0, x1, ldx1, y, ldy, rows, same01, same0y, same1y, partial);
	return launch_dev_dot_finalize(partial, pl.blocks, nx * n * n, P61, out, s);
}

hipError_t launch_devmfma_combine(const dm_plan &pl, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
				  const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
				  unsigned char *img, hipStream_t s)
{
	const int pair = a1 != nullptr;
	if (pl.form != 1 || (n != 8 && n != 16) || nterms < 1 || nterms > DM_MAX_TERMS || rows < 1 || pl.blocks < 1 || !img ||
	    pl.sets != (pair && n == 16 ? 2 : 1) || pl.ksteps != dm_combine_ksteps(n, nterms) ||
	    pl.image_bytes > dm_image_bytes_max() || pl.lds_bytes != pl.image_bytes)
		return hipErrorInvalidValue;
	DmCombineArgs g{};
	for (int t = 0; t < nterms; t++) {
		g.x[t] = x[t];
		g.ldx[t] = ldx[t];
		g.a0[t] = a0[t];
		g.a1[t] = pair ? a1[t] : nullptr;
	}
	g.z0 = z0;
	g.z1 = pair ? z1 : nullptr;
	g.ldz0 = ldz0;
	g.ldz1 = pair ? ldz1 : 0;
	const unsigned prep_grid = (unsigned)(pl.sets * DM_ND * 16 / 4);
	if (n == 16) {
		hipLaunchKernelGGL((k_dm_prep<16>), dim3(prep_grid), dim3(256), 0, s, g, pl.sets, pl.ksteps, img);
		if (pl.sets == 2)
			return combine_terms<16, 2>(nterms, pl, g, pair, rows, img, s);
		return combine_terms<16, 1>(nterms, pl, g, pair, rows, img, s);
	}
	hipLaunchKernelGGL((k_dm_prep<8>), dim3(prep_grid), dim3(256), 0, s, g, pl.sets, pl.ksteps, img);
	return combine_terms<8, 1>(nterms, pl, g, pair, rows, img, s);
}
