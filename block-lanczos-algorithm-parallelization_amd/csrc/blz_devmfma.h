/* blz_devmfma.h -- launchers of the device block algebra on the matrix cores (blz_devmfma.hip): X^T * Y (one or two left blocks)
 * and sum_t X_t * A_t (one or two outputs) at p = 2^61 - 1, n = 8 or 16, on a caller's strided u64 rows, as exact integer
 * contractions of base-256 digits on v_mfma_i32_16x16x64_i8.  The conventions are blz_devalg.h's; whether a call comes here is
 * decided by dm_decide() (blz_devmfma_plan.h), and the dm_plan it filled is what the launchers run.  C++ side only; not part of
 * the C ABI. */
#ifndef BLZ_DEVMFMA_H
#define BLZ_DEVMFMA_H

#include "blz_devalg.h"
#include "blz_devmfma_plan.h"

/* nx = 1: out[i * n + j] = sum_r x0[r * ldx0 + i] * y[r * ldy + j] mod p (x1 is not read); nx = 2: a second panel of n * n words
 * follows it, the same with x1.  Blocks that are the same pointer with the same stride are read once.  `partial` has room for
 * `max_blocks` rows of nx * n * n words (pl.blocks of them are written); a second launch adds the rows mod p into `out`.
 * Needs pl.form == 1 (rows >= 1, every base 16-byte aligned, every ld even). */
hipError_t launch_devmfma_dot(const dm_plan &pl, int n, long long rows, int nx, const u64 *x0, long long ldx0, const u64 *x1,
			      long long ldx1, const u64 *y, long long ldy, u64 *partial, int max_blocks, u64 *out, hipStream_t s);

/* z0[r * ldz0 + j] = sum_t sum_i x[t][r * ldx[t] + i] * a0[t][i * n + j] mod p; with a1 != NULL (the pair) z1 the same with
 * a1, and a NULL a0[t] / a1[t] is a zero panel.  `img` is device scratch of dm_image_bytes_max() bytes: a first launch writes
 * the coefficients' digit image there, the second reads it.  A wavefront reads its 16 rows of every term before it writes a
 * row of either output, and no other wavefront touches them: each output may BE one of the x[t].  Needs pl.form == 1. */
hipError_t launch_devmfma_combine(const dm_plan &pl, int n, long long rows, int nterms, const u64 *const *x, const long long *ldx,
				  const u64 *const *a0, const u64 *const *a1, u64 *z0, long long ldz0, u64 *z1, long long ldz1,
				  unsigned char *img, hipStream_t s);

#if defined(__HIPCC__)

typedef int dm_v4i __attribute__((ext_vector_type(4)));

/* The small device helpers below are restated from blz_dense_mfma.hip (mad_u64, fold61, digit_fragments, digit_fragment_pair,
 * fold_partial61, fold_shift): that file keeps its own copies and is not touched. */

/* weight of digit sum s in the folded result: 2^(8 s mod 61), applied as a 32-bit multiplier into L (shift < 32) or H */
__host__ __device__ constexpr int dm_fold_shift(int s) { return (8 * s) % 61; }

/* acc += a * b (32 x 32 -> 64, 64-bit add).  Plain C on purpose: the operands come straight out of an MFMA, and the compiler
 * pads the MFMA -> VALU read hazard only for instructions it can see (inline asm read stale accumulators here).  `b` is a
 * power of two the compiler must not recognise as one (it would shift and add: three instructions instead of one
 * v_mad_u64_u32), hence the opaque `one` of the kernels. */
MODP_DEV void dm_mad_u64(u64 &acc, u32 a, u32 b)
{
	acc += (u64)a * (u64)b;
}

/* value = L + H * 2^32 (L < 2^61, H < 2^56): fold mod 2^61 - 1 */
MODP_DEV u64 dm_fold61(u64 L, u64 H)
{
	const u64 P = (1ull << 61) - 1;
	const u64 lo = L + (H << 32), carry = lo < L;
	const u64 hi = (H >> 32) + carry;
	u64 x = (lo & P) + ((lo >> 61) | (hi << 3));	/* hi < 2^25: (hi << 3) < 2^28 */
	x = (x & P) + (x >> 61);
	return x >= P ? x - P : x;
}

MODP_DEV u64 dm_fold_partial61(u64 s)	/* s < 2^64 -> < 2^62, congruent mod 2^61 - 1 */
{
	return (s & ((1ull << 61) - 1)) + (s >> 61);
}

/* fragments of the 8 base-256 digits of 16 words: digit a of word q goes to byte q of frag[a] (4 dwords), biased by 128 */
MODP_DEV void dm_digit_fragments(const u64 *x, dm_v4i *frag)
{
#pragma unroll
	for (int d = 0; d < 4; d++) {
#pragma unroll
		for (int half = 0; half < 2; half++) {
			u32 w0 = (u32)(x[4 * d + 0] >> (32 * half)), w1 = (u32)(x[4 * d + 1] >> (32 * half));
			u32 w2 = (u32)(x[4 * d + 2] >> (32 * half)), w3 = (u32)(x[4 * d + 3] >> (32 * half));
			/* 4 x 4 byte transpose: t = bytes {w0.b0 w1.b0 w0.b1 w1.b1} ..., then pairs of 16-bit halves */
			const u32 t01l = __builtin_amdgcn_perm(w1, w0, 0x05010400u);
			const u32 t01h = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
			const u32 t23l = __builtin_amdgcn_perm(w3, w2, 0x05010400u);
			const u32 t23h = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
			const u32 a0 = __builtin_amdgcn_perm(t23l, t01l, 0x05040100u);
			const u32 a1 = __builtin_amdgcn_perm(t23l, t01l, 0x07060302u);
			const u32 a2 = __builtin_amdgcn_perm(t23h, t01h, 0x05040100u);
			const u32 a3 = __builtin_amdgcn_perm(t23h, t01h, 0x07060302u);
			frag[4 * half + 0][d] = (int)(a0 ^ 0x80808080u);
			frag[4 * half + 1][d] = (int)(a1 ^ 0x80808080u);
			frag[4 * half + 2][d] = (int)(a2 ^ 0x80808080u);
			frag[4 * half + 3][d] = (int)(a3 ^ 0x80808080u);
		}
	}
}

/* the same for two digits only: digits 2 * PR_ and 2 * PR_ + 1 of the 16 words -> out[0], out[1] (two fragments of the left
 * operand live at a time instead of eight) */
template <int PR_>
MODP_DEV void dm_digit_fragment_pair(const u64 *x, dm_v4i *out)
{
	constexpr int half = PR_ >> 1, hi = PR_ & 1;
#pragma unroll
	for (int d = 0; d < 4; d++) {
		const u32 w0 = (u32)(x[4 * d + 0] >> (32 * half)), w1 = (u32)(x[4 * d + 1] >> (32 * half));
		const u32 w2 = (u32)(x[4 * d + 2] >> (32 * half)), w3 = (u32)(x[4 * d + 3] >> (32 * half));
		const u32 t01 = __builtin_amdgcn_perm(w1, w0, hi ? 0x07030602u : 0x05010400u);
		const u32 t23 = __builtin_amdgcn_perm(w3, w2, hi ? 0x07030602u : 0x05010400u);
		out[0][d] = (int)(__builtin_amdgcn_perm(t23, t01, 0x05040100u) ^ 0x80808080u);
		out[1][d] = (int)(__builtin_amdgcn_perm(t23, t01, 0x07060302u) ^ 0x80808080u);
	}
}

#endif /* __HIPCC__ */
#endif
