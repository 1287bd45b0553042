/*
 * blz_devmfma_plan.h -- the host arithmetic of the device block algebra on the matrix cores (kernels: blz_devmfma.hip): the
 * ONE decision whether a call takes the matrix-core form, and the geometry of the launch it then makes (image layout, LDS,
 * workgroups).  Plain C, no HIP: blz_api.hip decides with it, blz_devmfma.hip launches with it, blz_devalg_plan reports it and
 * tests/host_sanitize_devmfma.c runs it under the sanitizers.  DESIGN.md section 26.
 */
#ifndef BLZ_DEVMFMA_PLAN_H
#define BLZ_DEVMFMA_PLAN_H

#include <stddef.h>
#include <stdint.h>

/* = BLZ_DEVOP_* of blz.h */
enum { DM_OP_DOT = 0, DM_OP_DOT_PAIR = 1, DM_OP_COMBINE = 2, DM_OP_COMBINE_PAIR = 3, DM_NOPS = 4 };

#define DM_MAX_TERMS 4			/* = BLZ_MAX_TERMS */
#define DM_ND 8				/* signed base-256 digit positions of a 61-bit multiplier */
#define DM_KMAX (8 * 16 * DM_MAX_TERMS)	/* the longest contraction of a recombination: K' = 8 n nterms bytes */
/* A digit sum is start + sum over K' of u * d with a byte u in [0, 255] and a signed digit d in [-128, 127], so it lies in
 * [start - K' * 255 * 128, start + K' * 255 * 127].  The start is the least one that keeps the lower end at 0 for the longest
 * K' launched; the upper end is then K' * 255 * 255 = 33 292 800 < 2^25. */
#define DM_START (DM_KMAX * 255 * 128)
#define DM_SUM_MAX (DM_START + DM_KMAX * 255 * 127)

#define DM_COMBINE_TILE_ROWS 16		/* rows of one MFMA tile: a wavefront's unit of work in a recombination */
#define DM_DOT_TILE_ROWS 64		/* rows one MFMA contracts in an inner product */
/* an inner product's int32 accumulators start at 2^30; a tile moves one by at most 8 digit pairs * 64 rows * 128 * 128 = 2^23,
 * so after 64 tiles it is still inside [2^29, 3 * 2^29] */
#define DM_DOT_FOLD_TILES 64
#define DM_DOT_THREADS 256
#define DM_LDS_PER_CU (160 * 1024)
#define DM_WAVES_PER_CU 16		/* what a recombination launch keeps resident on a CU */
#define DM_ROWS_OFF INT64_MAX		/* a threshold no row count reaches: that (call, width) stays on the vector ALU */

/* The rows from which a (call, width) takes the matrix-core form when BLZ_DEV_MFMA_MIN_ROWS is not set: the smallest measured
 * row count from which the form was faster at every larger one (profiles/device_mfma_cost.txt), and
 * DM_ROWS_OFF where there was none. */
static inline int64_t dm_default_min_rows(int op, int n)
{
	/* one MI355X, rows 2^12 .. 2^20 in steps of 4 and 1 911 130: every pair has such a row count.  The recombination was
	 * measured with 2 and 3 terms (its threshold is the larger of the two), the pair with the 3 terms of a Lanczos step */
	if (n == 16)
		return 65536;
	if (n != 8)
		return DM_ROWS_OFF;
	switch (op) {
	case DM_OP_DOT:
	case DM_OP_DOT_PAIR:
		return 65536;
	case DM_OP_COMBINE:
		return 1048576;
	case DM_OP_COMBINE_PAIR:
		return 262144;
	default:
		return DM_ROWS_OFF;
	}
}

typedef struct dm_env {
	int mfma;		/* the context's cfg.mfma (BLZ_NO_MFMA != 1) */
	int word_bytes;		/* of the context's residues */
	int p_is_m61;		/* p == 2^61 - 1 */
	int n;			/* block width of the device calls */
	int num_cu;
	int64_t min_rows[DM_NOPS][2];	/* [op][n == 16] */
} dm_env;

typedef struct dm_plan {
	int form;		/* 0 vector ALU, 1 matrix cores */
	int64_t min_rows;
	int tile_rows, wavefronts, fold_tiles;
	int64_t lds_bytes;
	/* the launch (form 1 only) */
	int threads, blocks;
	int sets, ksteps;	/* recombination: B images (1, or 2 for the pair at n = 16) and K steps of 64 bytes each */
	int64_t image_bytes;
} dm_plan;

/* (the layout functions are the kernels' too) */
#if defined(__HIPCC__)
#define DM_FN __host__ __device__ static inline
#else
#define DM_FN static inline
#endif

/* recombination image: [set][K step][digit position][lane][16 bytes] signed digits, then [set][digit position][16] int32 starts */
DM_FN int dm_combine_sets(int op, int n) { return op == DM_OP_COMBINE_PAIR && n == 16 ? 2 : 1; }
DM_FN int dm_combine_ksteps(int n, int nterms) { return n * nterms / 8; }
DM_FN int64_t dm_image_b_bytes(int sets, int ksteps) { return (int64_t)sets * ksteps * DM_ND * 64 * 16; }
DM_FN int64_t dm_image_bytes(int sets, int ksteps) { return dm_image_b_bytes(sets, ksteps) + (int64_t)sets * DM_ND * 16 * 4; }
/* the largest image: the pair at n = 16 with four terms, 2 * 8 * 8 KB + 1 KB = 132 096 bytes -- the context's scratch */
DM_FN int64_t dm_image_bytes_max(void) { return dm_image_bytes(2, dm_combine_ksteps(16, DM_MAX_TERMS)); }

/* offset of the 16 bytes lane `lane` reads for (set, K step, digit position), and of an accumulator start */
DM_FN int64_t dm_image_frag_at(int ksteps, int set, int ks, int dg, int lane)
{
	return ((((int64_t)set * ksteps + ks) * DM_ND + dg) * 64 + lane) * 16;
}
DM_FN int64_t dm_image_init_at(int sets, int ksteps, int set, int dg, int col)
{
	return dm_image_b_bytes(sets, ksteps) + (((int64_t)set * DM_ND + dg) * 16 + col) * 4;
}

/* LDS of the inner-product kernel: per wavefront the residues of NP products in the accumulator layout, three column sums and a
 * tile count */
static inline int64_t dm_dot_lds_bytes(int op, int n)
{
	const int np = op == DM_OP_DOT_PAIR && n == 16 ? 2 : 1, waves = DM_DOT_THREADS / 64;
	return (int64_t)waves * np * 4 * 64 * 8 + (int64_t)waves * 3 * 64 * 8 + (int64_t)waves * 8;
}

/* The decision and the launch geometry.  aligned16: every tall block's base is 16-byte aligned and every ld is even.
 * Returns 0, or -1 for an unknown op or nterms outside 1..DM_MAX_TERMS (then *out is untouched). */
static inline int dm_decide(const dm_env *e, int op, int64_t rows, int nterms, int aligned16, dm_plan *out)
{
	if (op < 0 || op >= DM_NOPS || nterms < 1 || nterms > DM_MAX_TERMS)
		return -1;
	dm_plan p = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	const int shape_ok = e->mfma && e->word_bytes == 8 && e->p_is_m61 && (e->n == 8 || e->n == 16);
	p.min_rows = shape_ok ? e->min_rows[op][e->n == 16] : DM_ROWS_OFF;
	if (!shape_ok || !aligned16 || rows < 1 || rows < p.min_rows) {
		*out = p;
		return 0;
	}
	p.form = 1;
	if (op == DM_OP_DOT || op == DM_OP_DOT_PAIR) {
		const int64_t ntiles = rows / DM_DOT_TILE_ROWS + (rows % DM_DOT_TILE_ROWS != 0), wpb = DM_DOT_THREADS / 64;
		int64_t blocks = ntiles / wpb + (ntiles % wpb != 0);
		/* two wavefronts per SIMD; one for the pair at n = 16 (its kernel's registers) */
		const int64_t cap = (int64_t)(e->num_cu > 0 ? e->num_cu : 1) * (op == DM_OP_DOT_PAIR && e->n == 16 ? 1 : 2);
		blocks = blocks > cap ? cap : blocks;
		p.tile_rows = DM_DOT_TILE_ROWS;
		p.fold_tiles = DM_DOT_FOLD_TILES;
		p.threads = DM_DOT_THREADS;
		p.blocks = (int)blocks;
		p.lds_bytes = dm_dot_lds_bytes(op, e->n);
	} else {
		p.sets = dm_combine_sets(op, e->n);
		p.ksteps = dm_combine_ksteps(e->n, nterms);
		p.image_bytes = dm_image_bytes(p.sets, p.ksteps);
		p.lds_bytes = p.image_bytes;
		/* DM_WAVES_PER_CU wavefronts per CU beside the images: workgroups of 4, 8 or 16 of them */
		p.threads = p.lds_bytes * 4 <= DM_LDS_PER_CU ? 256 : p.lds_bytes * 2 <= DM_LDS_PER_CU ? 512 : 1024;
		if (p.sets == 2 && p.threads > 512)
			p.threads = 512;	/* two chains need more than the 128 registers of a 1024-thread workgroup */
		const int64_t ntiles = rows / DM_COMBINE_TILE_ROWS + (rows % DM_COMBINE_TILE_ROWS != 0), wpb = p.threads / 64;
		int64_t blocks = ntiles / wpb + (ntiles % wpb != 0);
		const int64_t cap = (int64_t)(e->num_cu > 0 ? e->num_cu : 1) * (DM_WAVES_PER_CU / wpb);
		blocks = blocks > cap ? cap : blocks;
		p.tile_rows = DM_COMBINE_TILE_ROWS;
		p.fold_tiles = 0;
		p.blocks = (int)blocks;
	}
	p.wavefronts = p.blocks * (p.threads / 64);
	*out = p;
	return 0;
}

#endif
