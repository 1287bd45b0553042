/*
 * blz.h -- C ABI of libblz_hip.so: the block-Lanczos-mod-p hot path on MI355X (gfx950).
 *
 * The reference (T-amairi/block-lanczos-algorithm-parallelization) has no FFI or plugin seam:
 * its kernels are plain C functions inside sequential/lanczos_modp.c, parameterised by two
 * globals (`long n`, `u64 prime`, :39-40) and caller-owned flat arrays.  This header exports one
 * entry point per reference function on the hot path, with the globals folded into an opaque
 * per-GPU context.  File:line citations are relative to /root/reference/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no C++ or torch types cross the boundary.
 *   - every function returns 0 (BLZ_OK) or a negative BLZ_E* code; blz_last_error() holds the
 *     text the reference would have passed to errx() (thread-local, valid until the next call).
 *   - host blocks are row-major rows x n arrays of uint64_t canonical residues in [0,p), exactly
 *     the reference's `v[i*n + l]` layout (sequential/lanczos_modp.c:282-284) with the word
 *     widened from u32 to u64 (the reference's cap p <= 2^30-35, :189-193, is lifted to p < 2^62).
 *   - a context owns all device memory and one HIP stream; the caller owns every host pointer.
 *     One context per GPU, driven by one host thread at a time.
 *   - functions in the "host-side" section never touch the GPU and work on any machine.
 */
#ifndef BLZ_H
#define BLZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLZ_OK          0
#define BLZ_EINVAL     -1	/* bad argument / unsupported size */
#define BLZ_EIO        -2	/* file could not be opened / parsed */
#define BLZ_EFORMAT    -3	/* MatrixMarket type not "coordinate integer general" */
#define BLZ_ENOMEM     -4
#define BLZ_EHIP       -5	/* a HIP runtime call failed */
#define BLZ_ENOGPU     -6	/* no usable gfx950 device: there is NO CPU fallback */
#define BLZ_ECOMM      -7	/* RCCL failure */

#define BLZ_MAX_N      64	/* block width limit (one wavefront holds a block row) */
#define BLZ_MAX_RHS    16	/* right-hand sides of one bordered solve (blz_set_matrix_rhs_block) */

/* block selectors: the four N x n blocks of block_lanczos(), sequential/lanczos_modp.c:602-605 */
enum { BLZ_V = 0, BLZ_TMP = 1, BLZ_AV = 2, BLZ_P = 3 };
/* small n x n (or n) operands of one iteration, sequential/lanczos_modp.c:638-643 */
enum { BLZ_VTAV = 0, BLZ_VTAAV = 1, BLZ_WINV = 2, BLZ_D = 3 };

typedef struct blz_ctx blz_ctx;

const char *blz_last_error(void);
int blz_version(void);

/* ------------------------------------------------------------------ host-side (no GPU) */

/* struct sparsematrix_t, sequential/lanczos_modp.c:55-62: 0-based COO triplets in file order;
 * x already canonicalised as the loader does (below). */
typedef struct {
	int64_t nrows, ncols, nnz;
	int32_t *i, *j;
	uint32_t *x;
} blz_coo;

/* CSR of M (or of M^T): what the HIP SpMV streams.  row_ptr has rows+1 entries. */
typedef struct {
	int64_t rows, cols, nnz;
	uint32_t *row_ptr;
	int32_t *col_idx;
	uint32_t *val;		/* NULL = every entry is 1 (pattern path) */
} blz_csr;

/* sparsematrix_mm_load(), sequential/lanczos_modp.c:199-263: accepts only
 * "matrix coordinate integer general" (:216-221, BLZ_EFORMAT otherwise); entries are parsed as
 * C ints, stored into a u32 and reduced `% prime` (:238-243) -- negative entries therefore wrap
 * to 2^32-|x| before the reduction, exactly as in the reference and in checker_modp.c:170-175.
 * Unlike the reference, out-of-range indices are an error (BLZ_EIO) instead of undefined behaviour.
 * So -1 is stored as (2^32 - 1) % prime, which is p - 1 for no prime: a user who means the integer matrix mod p
 * wants blz_mm_load_signed below and a context in signed value mode (blz_set_values_signed). */
int blz_mm_load(const char *path, uint64_t prime, blz_coo *out);
/* Signed value mode: the same files, but x[k] is the entry's int32 BIT PATTERN (two's complement), to be read as the
 * residue a mod p by a context in signed value mode and by the *_signed checkers below.  No prime: nothing is reduced here.
 * An entry outside int32 is BLZ_EIO, never a silent wrap; int32 is the whole domain of the mode.  (For prime >= 2^32
 * blz_mm_load stores the same words: `% prime` is the identity on a u32.) */
int blz_mm_load_signed(const char *path, blz_coo *out);
/* Wide value mode: the same files and banner rules, but an entry is any decimal integer that fits an int64, sign included,
 * and what is stored is its canonical residue a mod prime (2 <= prime < 2^62): -1 is p - 1, p is 0, p + 5 is 5.  The residue
 * travels as two 32-bit limbs: the low one in out->x[k], the high one in (*x_hi)[k] -- an array parallel to x, to be handed to
 * blz_set_values_wide and freed with blz_values_free.  *x_hi is NULL when no residue reaches 2^32 (always so for prime < 2^32):
 * the triplets are then ordinary ones.  A token outside int64 is BLZ_EIO, naming the entry and its line, never a wrap. */
int blz_mm_load_wide(const char *path, uint64_t prime, blz_coo *out, uint32_t **x_hi);
void blz_values_free(uint32_t *x_hi);
void blz_coo_free(blz_coo *M);

/* Write triplets as a MatrixMarket "coordinate integer general" file (1-based, values as stored).  Used to hand a
 * synthetic matrix to programs that only read files (the reference binaries). */
int blz_mm_save_coo(const char *path, const blz_coo *M);

/* Seeded synthetic stand-in for a SuiteSparse matrix that is not on the box:
 * row r gets floor(nnz/R) + (r < nnz mod R) distinct uniform columns; values from
 * {1,1,1,2,3,-1,-2} (pattern=0, canonicalised like the loader does) or all 1 (pattern=1).
 * For prime >= 2^32 the stored words are the bit patterns of those values, i.e. what blz_mm_load_signed would store: the
 * same triplets serve a context in signed value mode unchanged (below 2^32 they are already reduced and do not). */
int blz_synth_coo(int64_t nrows, int64_t ncols, int64_t nnz, uint64_t seed, int pattern,
		  uint64_t prime, blz_coo *out);
/* The entries of that same matrix in rows [r0, r1) and columns [c0, c1), global indices, without making the rest
 * (every row is seeded by itself): a rank's own rows (c0 = 0, c1 = ncols) or own columns (r0 = 0, r1 = nrows) of a
 * matrix too large to hold whole -- config 5's 2e9 entries.  What the reference's MPI loader does with
 * the file (mpi/lanczos_modp.c:1841-1845). */
int blz_synth_coo_part(int64_t nrows, int64_t ncols, int64_t nnz, uint64_t seed, int pattern, uint64_t prime,
		       int64_t r0, int64_t r1, int64_t c0, int64_t c1, blz_coo *out);

/* A synthetic matrix WITH structure (never the headline workload): hot_pct % of a row's entries are drawn with
 * probability ~ 1/(c + 16) (heavy-tailed column degrees, dense columns first, as in a sieve relation matrix),
 * band_pct % uniformly from a band of `band` columns centred on r * C / R (correlated supports of neighbouring
 * rows), the rest uniformly.  Used to measure what the uniform stand-ins cannot show: the LDS-resident panel of
 * dense block rows and the per-XCD row ranges of the SpMV. */
int blz_synth_structured(int64_t nrows, int64_t ncols, int64_t nnz, uint64_t seed, int pattern, uint64_t prime,
			 int hot_pct, int band_pct, int64_t band, blz_coo *out);

/* COO -> CSR of M (transpose=0) or of M^T (transpose=1); duplicates are kept (they add,
 * as in the reference's scatter loop :277-286).  pattern!=0 drops the value array when all
 * values are 1. */
int blz_csr_from_coo(const blz_coo *M, int transpose, int pattern, blz_csr *out);
void blz_csr_free(blz_csr *A);

/* nnz-balanced contiguous row partition: bounds[0]=0 <= ... <= bounds[parts]=rows. */
int blz_partition_rows(const blz_csr *A, int parts, int64_t *bounds);

/* Locality reordering of both index spaces (host only).  Every step of the iteration is invariant under
 * permutations of the rows of v and of tmp (sums mod p are exact and order-free), so the solver is free to
 * renumber them: rows of M are sorted by their smallest column index, then columns by their smallest (new) row
 * index.  The entries that define the order then hit the same or the next block row as their neighbours
 * (shared L2 lines, two 64-byte rows per 128-byte fabric request) in BOTH products.  Measured on MI355X:
 * -5 % per iteration on the GL7d19-shape matrix, -9 % on the relat9 shape.
 * row_perm[r] / col_perm[c] = new index of row r / column c of M (arrays of nrows / ncols int32). */
int blz_reorder(const blz_coo *M, int32_t *row_perm, int32_t *col_perm);

/* blz_reorder with the densest rows / columns numbered first.  hot[0] (rows) and hot[1] (columns): in = the most a
 * panel can hold, out = how many were taken (0 when they hold less than min_share of the entries); share[] = the
 * fraction of the entries they hold.  The SpMV keeps the first hot[.] block rows of its operand in LDS. */
int blz_reorder_hot(const blz_coo *M, int32_t *row_perm, int32_t *col_perm, int64_t hot[2], double min_share,
		    double share[2]);
/* The renumbering the solver uses: blz_reorder_hot's hot rows / columns in front, and behind them the best of three
 * orders -- rows by smallest column (blz_reorder), the file's own order, rows by the mean of their columns -- judged on a
 * sample of windows of 4096 consecutive rows of each product by the number of distinct 128-byte lines of the operand
 * they touch (rows_per_line block rows share a line).  locality[t] = lines per gathered entry of product t (0: M * x,
 * 1: M^T * x) under the chosen order; 1.0 means no reuse to be had.  *kind (may be NULL): 0 smallest, 1 file order, 3 iterated barycentre sweeps,
 * 2 mean. */
int blz_reorder_auto(const blz_coo *M, int32_t *row_perm, int32_t *col_perm, int64_t hot[2], double min_share,
		     double share[2], int rows_per_line, double locality[2], int *kind);
/* entries of every row in ascending column order */
void blz_csr_sort_rows(blz_csr *A);

/* ---- the prepared matrix: everything blz_set_matrix needs that does not depend on the rank, made ONCE ----
 * (renumbering, CSR(M) and CSR(M^T) in the solver's numbering, nnz-balanced row partition of both sides).  The CLI's
 * main thread prepares for its G contexts; rank 0 of a multi-process job prepares, saves, and the other ranks load
 * (mmap: one copy of the pages per node).  Saved next to the matrix it is the binary cache of SURVEY 8(f)1: a second
 * run skips the renumbering and the CSR builds.  sequential/lanczos_modp.c:199-263 is what it stands in front of.
 *   reorder        0 keep the file's numbering, 1 scored choice (blz_reorder_auto), 2 round 1's order
 *   chunks         pieces per exchange (1 for one rank)
 *   rows_per_line  block rows of the context per 128-byte line (128 / (width in HBM * word bytes), at least 1)
 *   hot_cap        block rows the LDS panel can hold (0: none); only used with one rank and one piece
 * `key` ties a cache file to its inputs (the CLI uses blz_file_hash of the matrix ^ prime, width, ranks, ...): a
 * load with another key fails with BLZ_EFORMAT and the caller prepares afresh. */
typedef struct blz_prepared blz_prepared;
int blz_prepare(const blz_coo *M, int right, int nranks, int chunks, int reorder, int rows_per_line, int64_t hot_cap,
		double min_share, blz_prepared **out);
/* One rank's prepared matrix from that rank's share alone: row_part / col_part = the entries of M in its rows / in its
 * columns (global indices), the caller's partition (bounds: nranks + 1 ascending values from 0 to the dimension), the
 * caller's numbering (no renumbering).  Only blz_set_matrix_prepared(ctx, P, rank) with that rank accepts it; it cannot
 * be saved.  No process holds the whole matrix -- the reference's MPI variant works that way too
 * (mpi/lanczos_modp.c:1841-1900). */
int blz_prepare_rank(const blz_coo *row_part, const blz_coo *col_part, int64_t nrows, int64_t ncols, int64_t nnz_total,
		     int right, int rank, int nranks, int chunks, const int64_t *row_bounds, const int64_t *col_bounds,
		     blz_prepared **out);
int blz_prepared_save(const blz_prepared *P, const char *path, uint64_t key);
int blz_prepared_load(const char *path, uint64_t key, blz_prepared **out);
void blz_prepared_free(blz_prepared *P);
/* the row partition: bounds0 / bounds1 [nranks + 1] of side 0 (rows of v) / side 1 (rows of tmp), rows of a padded slab per side */
int blz_prepared_layout(const blz_prepared *P, int64_t *bounds0, int64_t *bounds1, int64_t stride[2]);
/* what P was prepared for (any pointer may be NULL) */
int blz_prepared_describe(const blz_prepared *P, int *right, int *nranks, int *chunks);
/* rank `rank`'s rows of M (t = 0) or of M^T (t = 1) as a CSR of its own, columns rewritten to positions in the gathered
 * operand (what blz_shard_matrix returns in slabs[t]) */
int blz_prepared_slab(const blz_prepared *P, int rank, int t, blz_csr *slab);
/* The matrix of product t in its SHORT-SIDE form (tall / wide matrices on several ranks): the transpose of this rank's
 * rows of the other orientation.  Rows = the padded rank-major numbering of the output side (nranks x stride), columns =
 * row numbers inside this rank's own slab of the operand: the rank multiplies it by its OWN slab (nothing is gathered)
 * and a reduce-scatter of the full-length partial products replaces the all-gather of the long block
 * (mpi/lanczos_modp.c:1108-1124 reduces partial products too, through rank 0). */
int blz_prepared_slab_short(const blz_prepared *P, int rank, int t, blz_csr *out);
/* 64-bit content hash of a file (0 on error) */
uint64_t blz_file_hash(const char *path);

/* What rank `rank` of `nranks` keeps of M for the solve (right=0: x*M=0, right=1: M*x=0).
 * "Side 0" is the row space of v/Av/p, "side 1" that of tmp (sequential/lanczos_modp.c:592-593).
 *   bounds0/bounds1 [nranks+1]  nnz-balanced row partition of each side
 *   stride[2]                   rows of a (padded) slab of each side, a multiple of `chunks`
 *   slabs[0] = this rank's rows of M, slabs[1] = its rows of M^T, column indices already rewritten to positions
 *              in the gathered operand of the opposite side:  with piece = stride/chunks, row q of rank g's slab
 *              sits at  (q / piece) * (nranks * piece) + g * piece + (q % piece)  -- piece-major, so that
 *              all-gather number k (piece k of every slab) lands contiguously and the product can start on it
 *              while piece k+1 is in flight.  chunks = 1 gives the plain rank-major padded layout
 *              g * stride + q; one rank gives the identity.
 * This is the whole multi-GPU data layout; blz_set_matrix uploads exactly these slabs. */
int blz_shard_matrix(const blz_coo *M, int right, int rank, int nranks, int chunks, blz_csr slabs[2],
		     int64_t *bounds0, int64_t *bounds1, int64_t stride[2]);

/* rng_state/random64(), sequential/lanczos_modp.c:67-87, and the initialisation
 * `v[i] = random64() % prime` in row-major order (:624-625). */
void blz_rng_seed(uint64_t state[4]);
uint64_t blz_rng_next(uint64_t state[4]);
int blz_rng_fill(uint64_t *v, int64_t words, uint64_t prime);

/* save_vector_block(), sequential/lanczos_modp.c:673-686: MatrixMarket "array integer general",
 * the same fixed comment line, column-major "%d" lines (words >= 2^32, which the reference
 * cannot produce, are written as unsigned decimals). */
int blz_save_block(const char *path, int64_t nrows, int n, const uint64_t *v);

/* checker_modp.c:81-204 widened to u64 words (the reference's checker parses kernel entries with "%d" into a
 * u32, so it cannot verify p > 2^31-1): loads the kernel block (MatrixMarket "array integer general", column-major,
 * rows must equal the matrix's rows -- or columns with right!=0, :99-124), rejects entries >= prime (:150),
 * computes y = x^T M (or M x) mod p and returns
 *   0 = OK, 1 = kernel vectors are all zero (:155-161), 2 = y != 0 (:199-203); bad_row and bad_col locate the first
 * non-zero word.  Negative returns are BLZ_E* errors (file, format, dimension mismatch). */
int blz_check_kernel(const char *matrix_path, const char *kernel_path, uint64_t prime, int right,
		     int64_t *bad_row, int *bad_col);
/* The same for the integer matrix mod p: the matrix is read with blz_mm_load_signed and an entry a stands for a mod p
 * (-1 is p - 1).  prime < 2^62.  Same return values. */
int blz_check_kernel_signed(const char *matrix_path, const char *kernel_path, uint64_t prime, int right,
			    int64_t *bad_row, int *bad_col);
/* The same for a matrix with wide entries: read with blz_mm_load_wide, every entry a residue below prime < 2^62. */
int blz_check_kernel_wide(const char *matrix_path, const char *kernel_path, uint64_t prime, int right,
			  int64_t *bad_row, int *bad_col);

/* Rank of a kernel block file (MatrixMarket "array integer general", column-major, as blz_save_block writes it) mod
 * prime: *rank = rank of its *cols columns, found by a row-by-row reduced echelon that stops once the rank equals the
 * column count.  No reference counterpart (checker_modp.c only tests v != 0 and x^T M = 0).  Host only, no GPU. */
int blz_check_independent(const char *kernel_path, uint64_t prime, int *rank, int *cols);

/* A right-hand side for blz_set_matrix_rhs (no reference counterpart: the reference finds kernel vectors only).  Reads a
 * MatrixMarket "array integer general" file of len x 1 entries, the format blz_save_block writes, into b[0..len).
 * Entries are signed decimal integers taken as TRUE residues: -1 becomes p - 1.  This is deliberately NOT the matrix
 * loader's wrap through a u32 (blz_mm_load, above), which restates a quirk of the reference's parser and has no meaning
 * for a vector of residues below p < 2^62 -- and not blz_save_block's "%d" rendering of words from 2^31 to 2^32 - 1
 * either: write such words as plain decimals.  A banner that is not "array integer general" is BLZ_EFORMAT; a size line
 * other than len x 1, an entry that does not parse or has 20 digits or more, and trailing entries are BLZ_EIO. */
int blz_rhs_load(const char *path, uint64_t prime, int64_t len, uint64_t *b);

/* Several right-hand sides for blz_set_matrix_rhs_block: an "array integer general" file of len x k entries, column-major
 * as blz_save_block writes a block, 1 <= k <= kmax, entries as in blz_rhs_load (signed, true residues).  Fills
 * b[r * k + i] = entry r of right-hand side i (row-major; room for len * kmax words) and *k.  With b == NULL only the
 * size line is read: *k receives its column count whenever the row count is len (len < 0: any), also when that count
 * exceeds kmax and the call fails.  Errors as blz_rhs_load; a column count outside 1..kmax is BLZ_EIO. */
int blz_rhs_load_block(const char *path, uint64_t prime, int64_t len, int kmax, int *k, uint64_t *b);

/* Host check of a solution file against a right-hand side file: x (len x 1, as blz_save_block writes it, entries below
 * prime) and b (as blz_rhs_load reads it) with M x == b (right != 0: x has M's column count, b its row count) or
 * x M == b (right == 0) mod prime, by unreduced 128-bit sums like blz_check_kernel.  Returns 0 = equal, 2 = not equal
 * (*bad_row, may be NULL = the first word of the product that differs from b), or a negative BLZ_E* code. */
int blz_check_solution(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime, int right,
		       int64_t *bad_row);

/* The same for k right-hand sides: b has k <= BLZ_MAX_RHS columns (blz_rhs_load_block) and x the same k columns (as
 * blz_save_block writes them).  status[i] (room for BLZ_MAX_RHS): 0 = column i is equal, 2 = not equal (bad_row[i], when
 * bad_row is not NULL, = the first word that differs), 3 = the x column is all zero (an unsolved system, not compared).
 * Returns k, or a negative BLZ_E* code. */
int blz_check_solution_block(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime, int right,
			     int *status, int64_t *bad_row);
/* Both for the integer matrix mod p (blz_mm_load_signed; an entry a stands for a mod p): same arguments and returns. */
int blz_check_solution_signed(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime, int right,
			      int64_t *bad_row);
int blz_check_solution_block_signed(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime,
				    int right, int *status, int64_t *bad_row);
/* Both for a matrix with wide entries (blz_mm_load_wide): same arguments and returns. */
int blz_check_solution_wide(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime, int right,
			    int64_t *bad_row);
int blz_check_solution_block_wide(const char *matrix_path, const char *rhs_path, const char *x_path, uint64_t prime,
				  int right, int *status, int64_t *bad_row);

/* TEST HOOKS, not part of the supported interface (they may change or go with the layout they describe; callers use
 * blz_set_rhs_ranks): two pieces of host arithmetic of the bordered solve on several ranks, visible so that tests can hold
 * them against a restatement and run them under a sanitizer in a program of their own.
 * blz_gathered_position: row `row` (solver's numbering) of a block partitioned by bounds[0..nranks] belongs to the rank g with
 * bounds[g] <= row < bounds[g + 1] (*owner), is row q = row - bounds[g] of that rank's slab (*local), and sits at
 *     (q / piece) * (nranks * piece) + g * piece + q % piece,   piece = stride / chunks,
 * in the gathered operand (the return value; the layout blz_shard_matrix describes; the identity for one rank).  owner and
 * local may be NULL.  Negative = BLZ_EINVAL (row outside the bounds, stride not a multiple of chunks).
 * blz_rhs_cut: the rows [first, first + count) in the solver's numbering of the len x k right-hand sides b (row-major,
 * original numbering; perm[r] = solver's number of row r, NULL = identity) as count x kp words, zero padded -- what one rank
 * keeps on its device.  out has room for max(count, 1) * kp words.  A word of b that is not below prime, in anybody's rows,
 * is BLZ_EINVAL. */
int64_t blz_gathered_position(const int64_t *bounds, int nranks, int64_t stride, int chunks, int64_t row, int *owner,
			      int64_t *local);
int blz_rhs_cut(const uint64_t *b, int64_t len, int k, int kp, uint64_t prime, const int32_t *perm, int64_t first, int64_t count,
		uint64_t *out);

/* Checkpoints (openMP/lanczos_modp.c:571-676, :933-940, :1013-1022).  blz_checkpoint_save writes
 * one binary file atomically (tmp + rename): v, p, iteration count, prime, n, shape.
 * The *_ref_text pair reads/writes the reference's five text files (v.txt tmp.txt Av.txt p.txt
 * verbosity.txt) in `dir` so that runs can be handed over in either direction (p < 2^32 only). */
int blz_checkpoint_save(const char *path, uint64_t prime, int n, int right, int64_t nrows,
			int64_t iterations, const uint64_t *v, const uint64_t *p);
int blz_checkpoint_load(const char *path, uint64_t prime, int n, int right, int64_t nrows,
			int64_t *iterations, uint64_t *v, uint64_t *p);
int blz_checkpoint_save_ref_text(const char *dir, int n, int64_t nrows, int64_t ncols,
				 int64_t iterations, double start, double now, const uint64_t *v,
				 const uint64_t *tmp, const uint64_t *Av, const uint64_t *p);
int blz_checkpoint_load_ref_text(const char *dir, int n, int64_t nrows, int64_t ncols,
				 int64_t *iterations, uint64_t *v, uint64_t *p);

/* ------------------------------------------------------------------------- device side */

int blz_device_count(void);	/* 0 when no GPU is visible; never fails */

/* Replaces the globals `n` and `prime`.  Fails with BLZ_ENOGPU when there is no device:
 * the product has no CPU path.  2 <= prime < 2^62, 1 <= n <= BLZ_MAX_N. */
int blz_create(blz_ctx **out, int device, uint64_t prime, int n);
void blz_destroy(blz_ctx *ctx);
int blz_word_bytes(const blz_ctx *ctx);	/* 4 if prime < 2^32 else 8: width of a residue in HBM */

/* Signed value mode (opt-in, sticky): every matrix this context is given afterwards -- blz_set_matrix, _prepared, the
 * _rhs* families, blz_prepare_for -- carries in x the int32 bit pattern of its entries (blz_mm_load_signed), and an entry a
 * means the residue a mod p.  Without it x is a u32 as blz_mm_load stores it.  Must be called before a matrix is set:
 * BLZ_EINVAL once one is resident.  The stream, palette, CSR and cache layouts are the same in both modes; blz_prepare_key
 * mixes the mode in, so a cache written in one mode is never loaded in the other.  Checkpoints hold v and p, not the
 * matrix: the mode is not recorded in them.  blz_values_signed: 0 / 1 = the mode of the context. */
int blz_set_values_signed(blz_ctx *ctx, int on);
int blz_values_signed(const blz_ctx *ctx);
/* 1 when that slab (arguments as blz_slab_plan; the short-side slab of a product in that form) runs the signed
 * instantiations of the SpMV kernels, 0 when it runs the unsigned ones -- any slab of an unsigned context, a slab without
 * negative entries, and every slab of 4-byte words (values canonicalised at upload) -- negative = BLZ_EINVAL. */
int blz_slab_signed(const blz_ctx *ctx, int transpose, int piece);

/* Wide value mode (opt-in, per matrix): any residue below p as a matrix entry.  x_hi[k] is the high limb of entry k of the
 * triplets that the NEXT matrix-setting call (blz_set_matrix, blz_set_matrix_rhs, blz_set_matrix_rhs_block) is given: the
 * entry is x[k] + 2^32 * x_hi[k], a canonical residue (BLZ_EINVAL from that call otherwise).  The pointer is borrowed until
 * that call returns and is consumed by it.  Must be called before a matrix is set.  BLZ_EINVAL: an nnz that does not match
 * (reported by the matrix-setting call), a resident matrix, a context in signed value mode, and a context with a
 * communicator, a loopback group or BLZ_FORCE_COMM -- a wide matrix lives on one rank in one piece (so does nranks > 1 in
 * the matrix-setting call).  While high limbs are pending, blz_set_matrix_prepared and the several-rank form of
 * blz_set_matrix_rhs_ranks answer BLZ_EINVAL (they cannot carry them) and leave them pending.  A matrix-setting call that
 * fails leaves the context out of the mode.  A high array of zeros is accepted: the matrix is then prepared exactly as an
 * ordinary one.  x_hi = NULL clears the mode.  The SpMV of a slab with wide entries runs the plain form only
 * (no staged and no panel form); blz_prepared_save refuses a prepared object that carries high limbs.  Checkpoints hold v
 * and p, not the matrix: the mode is not recorded in them.  blz_values_wide: 0 / 1 = the mode of the context. */
int blz_set_values_wide(blz_ctx *ctx, const uint32_t *x_hi, int64_t nnz);
int blz_values_wide(const blz_ctx *ctx);
/* 1 when that slab (arguments as blz_slab_plan) runs the wide instantiations of the SpMV kernels, 0 when it runs the
 * unsigned ones -- a slab without an entry of 2^32 or more, and every slab of 4-byte words -- negative = BLZ_EINVAL. */
int blz_slab_wide(const blz_ctx *ctx, int transpose, int piece);

/* Upload M for the solve x*M=0 (right=0) or M*x=0 (right=1), as block_lanczos(M, n, transpose)
 * receives it (sequential/lanczos_modp.c:585).  Builds CSR(M) and CSR(M^T) on the host, keeps
 * this rank's nnz-balanced row slabs, allocates the four blocks and zeroes them (:617-622).
 * rank/nranks = 0/1 for a single GPU. */
int blz_set_matrix(blz_ctx *ctx, const blz_coo *M, int right, int rank, int nranks);

/* Device matrix: the same matrix from triplets that live on the context's GPU -- CSR(M) and CSR(M^T)
 * are built there (check + histogram, scan, scatter, palette: csrc/blz_devmat.hip) and the triplets never visit the host.
 * blz_set_matrix_device means what blz_set_matrix(ctx, M, right, 0, 1) means for the same triplets; afterwards every call
 * that works on a one-rank context works (blz_set_rhs / blz_set_rhs_block want the extra empty line in nrows / ncols).
 *   i, j       nnz zero-based indices each, contiguous, idx_bytes = 4 (int32) or 8 (int64: rows 0 and 1 of the indices of a
 *              torch sparse COO tensor).  Duplicate (i, j) pairs are separate entries that add up.
 *   x          val_bytes = 0 with x == NULL: every entry is 1; 4: uint32_t residues; 8: uint64_t residues.  Every value is
 *              below p.  Entries that are all 1 give a pattern slab, 8-byte values of which one reaches 2^32 a wide slab
 *              (blz_values_wide() == 1, the limits of wide value mode: at most 2^30 entries per row and column), 8-byte
 *              values that are all below 2^32 exactly what the 4-byte form gives.
 *   bounds     nrows, ncols < 2^31, nnz < 2^32 - 1.
 * The caller's numbering is kept: the context is what one created under BLZ_NO_REORDER=1 is after blz_set_matrix -- no
 * permutation (device blocks go in and out as they are), blz_locality reports 1.0 / kind 0, no panel, no hot rows.  The
 * scored locality renumbering stays a host feature.
 * The call is ordered after what the caller has enqueued on `stream` (NULL: the null stream) and synchronises the host: it
 * reads back the counts of the check pass, the two row_ptr arrays (the outlier lists and the staged plans are made from them on
 * the host, as ever) and at most 256 palette values, and returns when the matrix is resident.  The caller's arrays are never
 * written and not referenced after the return.
 * BLZ_EINVAL, by name, before anything is enqueued: idx_bytes / val_bytes other than the above, x and val_bytes disagreeing, a
 * pointer not aligned to its element or not inside ONE allocation of the context's device for its whole range, a capturing
 * stream, a context in signed value mode, pending high limbs (blz_set_values_wide), a matrix on several ranks, a
 * communicator, a loopback group, BLZ_FORCE_COMM.  BLZ_EINVAL with the counts in the message after the check pass: indices
 * outside [0, nrows) / [0, ncols) (any int64 index of 2^31 or more or below 0 included) and values not below p; no index
 * is used as an address before it has been checked and nothing is scattered before the host has read the counts as zero.
 * A refused or invalid call leaves the context exactly as it was: the matrix that was resident still applies.  A failure
 * after that point (out of memory, a HIP error) leaves the context WITHOUT a matrix.
 *   blz_set_matrix_upload    host triplets through the same build: they are copied into temporary device buffers.  The same
 *                            refusals, and those of blz_set_matrix for the blz_coo itself.  (The CLI's --device-build.)
 *   blz_matrix_device_built  1 when the resident matrix was built on the device, 0 otherwise */
int blz_set_matrix_device(blz_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j, int idx_bytes,
			  const void *x, int val_bytes, int right, void *stream);
int blz_set_matrix_upload(blz_ctx *ctx, const blz_coo *M, int right);
int blz_matrix_device_built(const blz_ctx *ctx);

/* Ordered device matrix: the device build with the rows and columns renumbered on the GPU first
 * (csrc/blz_devorder.hip).  order == 0 is blz_set_matrix_device / blz_set_matrix_upload in every respect; order == 1 means what
 * blz_set_matrix means on a context created under BLZ_REORDER_PLAIN=1 BLZ_NO_PANEL=1: the numbering is blz_reorder(M)'s, word
 * for word -- rows sorted stably by their smallest column (rows without entries take the key ncols and come last, ties stay
 * in ascending original index), then columns sorted the same way by their smallest NEW row -- with no hot rows and no
 * panel; blz_locality reports 1.0 / kind 0.  The key is a minimum and the sort is stable, so the numbering has one answer
 * whatever the schedule.  The argument decides: BLZ_NO_REORDER is not consulted.  Any other order is BLZ_EINVAL.
 * Refusals are those of the unordered calls, all before anything is enqueued; entries that are invalid give the unordered
 * call's message with its counts, and the resident matrix stays in place and still applies.  No index is used as an address
 * before it has been compared with its bound, in the minimum passes and the relabel pass included.
 * Afterwards the context carries the numbering as a host-renumbered one does: host blocks, device blocks, checkpoints,
 * blz_owner_of_row, blz_set_rhs*, blz_set_rhs_device and blz_solution_device speak the ORIGINAL numbering, and nothing of it
 * shows.  A matrix without entries keeps the identity.  Transient device memory: 8 bytes per entry (the relabelled
 * triplets, for the length of the build) and 32 bytes per row or column of the longer side (keys, the two permutations, the
 * sort's buffers and counters, freed before the CSRs are allocated); the two permutations are copied to the host once.
 * The caller's arrays are never written.  One rank; no prepared object, no cache.
 *   blz_matrix_device_order  1 when the resident matrix was built on the device with order 1, 0 otherwise (a host-built
 *                            matrix or no matrix included) */
int blz_set_matrix_device_ordered(blz_ctx *ctx, int64_t nrows, int64_t ncols, int64_t nnz, const void *i, const void *j,
				  int idx_bytes, const void *x, int val_bytes, int right, int order, void *stream);
int blz_set_matrix_upload_ordered(blz_ctx *ctx, const blz_coo *M, int right, int order);
int blz_matrix_device_order(const blz_ctx *ctx);

/* Device right-hand sides: the two ends of M x = b / x M = b on memory of the context's GPU, so that a
 * solve whose matrix came from blz_set_matrix_device needs nothing tall on the host.  The 64 / 32-bit twins follow the device
 * blocks' pattern (the ...32 forms: contexts of 4-byte words, blz_word_bytes(ctx) == 4, p < 2^32).  A plain single rank.
 *
 * blz_set_rhs_device means what blz_set_rhs_block(ctx, k, a host copy of b) means (k == 1: what blz_set_rhs means): the
 * border it leaves is that call's byte for byte, and so is every later product, iteration, checkpoint and solution.
 *   b          blz_rows(ctx, BLZ_TMP) rows of k words, row-major, ORIGINAL numbering, row stride ldb >= k words; words
 *              k .. ldb-1 of a row are never read.  All words below p.  Never written, not referenced after the return.
 *   the matrix already set with the k empty last rows (right == 0) / columns, by blz_set_matrix, _prepared, _device or _upload.
 * One kernel gathers b through the device copy of the numbering into a FRESH border (narrowed to the context's word, zero
 * padded) and counts the words that are not below p; the call synchronises the host, reads the count, and swaps the border in
 * only when it is zero.  BLZ_EINVAL by name, before anything is enqueued: no matrix, k outside 1..min(n, BLZ_MAX_RHS), ldb < k,
 * a NULL / host / misaligned pointer, a range ((rows - 1) * ldb + k words) that leaves its allocation, a capturing stream, a
 * matrix not set for one rank in one piece, a communicator, a loopback group, BLZ_FORCE_COMM, device blocks on ranks, border
 * lines that are not empty, and (the 32-bit twin) a context of 8-byte words.  After the pass: "N words of b are not below p".
 * A refused or invalid call leaves the context exactly as it was: the border that was resident still applies.
 *
 * blz_solution_device means what blz_solution_block means for every k, 1 included: the same state before, the same statuses
 * (status: a HOST array of BLZ_MAX_RHS ints), the same V and TMP afterwards.
 *   x          device memory, (blz_rows(ctx, BLZ_V) - k) rows of k words, row stride ldx >= k, original numbering; words
 *              past k of a row are never written.  Unsolved systems give zero columns; when the verification fails every
 *              status is 2 and x is untouched.
 * The kernel basis, the k x n border words and the small elimination go through the host as in blz_solution_block (the call
 * synchronises); the rows of V leave the slab through one kernel, ordered on `stream` like the device blocks. */
int blz_set_rhs_device(blz_ctx *ctx, int k, const uint64_t *b, int64_t ldb, void *stream);
int blz_set_rhs_device32(blz_ctx *ctx, int k, const uint32_t *b, int64_t ldb, void *stream);
int blz_solution_device(blz_ctx *ctx, uint64_t *x, int64_t ldx, int *status, void *stream);
int blz_solution_device32(blz_ctx *ctx, uint32_t *x, int64_t ldx, int *status, void *stream);

/* The same with the rank-independent work done once and shared (blz_prepare / blz_prepared_load above):
 *   blz_prepare_for   prepares M with the parameters THIS context wants (pieces per exchange from the slab sizes and
 *                     BLZ_AG_CHUNKS, renumbering, panel capacity from its block width and word size)
 *   blz_prepare_key   the cache key for those parameters and a content hash of the matrix
 *   blz_set_matrix_prepared  cuts rank `rank`'s slabs out of P and uploads them (P stays the caller's) */
int blz_prepare_for(const blz_ctx *c, const blz_coo *M, int right, int nranks, blz_prepared **out);
uint64_t blz_prepare_key(const blz_ctx *c, uint64_t content_hash, int64_t mrows, int64_t mcols, int64_t nnz, int right,
			 int nranks);
int blz_set_matrix_prepared(blz_ctx *c, const blz_prepared *P, int rank);
/* Solve M x = b (right != 0; b has M->nrows words) or x M = b (right == 0; b has M->ncols words), all words below p, as
 * kernel vectors of the bordered operator M' = [M | b] resp. [M ; b] with a non-zero last coordinate.  b is NOT stored
 * in the matrix (its values are u32; b holds residues below p < 2^62): M is prepared with the dimension raised by one --
 * an empty column resp. row, so every layout is sized for it and blz_rows(ctx, BLZ_V) reports one more row, the border
 * row, last in the original numbering -- and b stays on the device as a dense border that two kernels apply behind
 * each product (blz_spmv included):  tmp[r, :] += b[r] * v[border, :]  after the product that writes the rows of tmp,
 * Av[border, :] = sum_r b[r] * tmp[r, :]  after the other.  Iterations, checkpoints, blz_final_check, blz_kernel_basis
 * work as on any matrix; the second product runs without the fused inner products (blz_slab_plan reports fused == 0).
 * One rank only: with nranks > 1, a communicator or a loopback group attached the call fails with BLZ_EINVAL (several ranks:
 * blz_set_rhs_ranks, below).
 *   blz_set_matrix_rhs  the one-call form (prepare, upload, set the border)
 *   blz_set_rhs         sets the border on a context whose matrix the CALLER has set with the extra empty last row
 *                       (right == 0) / column (right != 0), e.g. through blz_prepare_for / blz_prepared_load /
 *                       blz_set_matrix_prepared (the CLI's --cache); b has blz_rows(ctx, BLZ_TMP) words
 *   blz_has_rhs         1 when the context carries a border
 * Setting a matrix again drops the border.
 *
 * Up to BLZ_MAX_RHS right-hand sides share ONE run: M X = B (right) / X M = B as kernel vectors of [M | B] / [M ; B], the
 * dimension raised by k, 1 <= k <= min(n, BLZ_MAX_RHS).  b = rows x k words, row-major (word [r * k + i] = entry r of
 * right-hand side i), all below p.  The two border kernels run once per product for all k columns.
 *   blz_set_matrix_rhs_block  the one-call form
 *   blz_set_rhs_block         for a matrix the caller has set with the k extra empty last rows / columns
 *   blz_rhs_count             0 without a border, 1 after blz_set_rhs / blz_set_matrix_rhs, k after the block forms
 * k == 1 is the single border above in every respect.  Same refusals (BLZ_EINVAL) as for one right-hand side.
 *
 * Several ranks -- nranks > 1 with an RCCL communicator, a loopback group, or BLZ_FORCE_COMM=1 on one rank -- go through two
 * entry points of their own (the four above keep their refusals):
 *   blz_set_matrix_rhs_ranks  the one-call form: M prepared for nranks with the dimension raised by k, rank `rank`'s slabs,
 *                             then the border.  It plans no short-side product, whatever BLZ_SHORT_SIDE says.
 *   blz_set_rhs_ranks         the border for a matrix the caller has set for its rank with the k empty last rows / columns
 *                             (blz_set_matrix_prepared)
 * b is the WHOLE right-hand side on every rank (rows x k words, row-major, below p), 1 <= k <= min(n, BLZ_MAX_RHS); a rank
 * keeps its own rows of it.  Both are collective: every rank checks the border rows it owns for emptiness and the verdict is
 * summed over the ranks, so either all ranks succeed or all fail.  On a plain single rank they are blz_set_rhs_block.
 * Per product and rank: the border update runs on the rank's slab of tmp with the k border rows read from the gathered
 * operand (nothing more is exchanged); the border dot runs over the rank's own rows, its k x n words are all-reduced (one
 * more small collective per iteration) and the rank that owns border row i stores it.  The border rows may sit on different
 * ranks.  blz_iterate, blz_spmv, blz_final_check, blz_kernel_basis, snapshots work as on any several-rank context;
 * blz_solution and blz_solution_block become collective there (every rank the same status; each writes only the rows of x it
 * owns, like blz_get_block, and leaves the rest of x untouched).
 * Refused with BLZ_EINVAL: external-exchange mode (and blz_set_exchange_mode(ctx, 1) afterwards); a matrix whose short-side
 * form is active (the border rows of the operand are not gathered in that form); border rows that are not empty; words not
 * below p; k out of range. */
int blz_set_matrix_rhs_ranks(blz_ctx *ctx, const blz_coo *M, int right, int k, const uint64_t *b, int rank, int nranks);
int blz_set_rhs_ranks(blz_ctx *ctx, int k, const uint64_t *b);
int blz_set_matrix_rhs_block(blz_ctx *ctx, const blz_coo *M, int right, int k, const uint64_t *b);
int blz_set_rhs_block(blz_ctx *ctx, int k, const uint64_t *b);
int blz_rhs_count(const blz_ctx *ctx);
int blz_set_matrix_rhs(blz_ctx *ctx, const blz_coo *M, int right, const uint64_t *b);
int blz_set_rhs(blz_ctx *ctx, const uint64_t *b);
int blz_has_rhs(const blz_ctx *ctx);

/* The solver renumbers rows internally (blz_reorder; BLZ_NO_REORDER=1 disables it).  Nothing of it is visible
 * through this ABI: blz_set_block / blz_get_block / blz_init_v / checkpoints all speak the ORIGINAL row numbering,
 * and results are bit-identical either way.  With nranks > 1 a rank's slab is a set of original rows that need
 * not be contiguous; blz_owner_of_row tells which rank holds a given original row of a block. */
int blz_owner_of_row(const blz_ctx *ctx, int block, int64_t row);

/* Block rows of the operand of product `transpose` (0: M * x, 1: M^T * x) that the SpMV keeps in LDS: the densest
 * columns (rows for the transpose) of a heavy-tailed matrix, numbered first by the solver's internal renumbering.
 * 0 for matrices without such structure, with several ranks, or with BLZ_NO_PANEL=1.  *share (may be NULL) = the
 * fraction of the entries those block rows serve. */
int64_t blz_panel_rows(const blz_ctx *c, int transpose, double *share);

/* What the renumbering found: locality[t] = distinct 128-byte lines of the operand per gathered entry in windows of 4096
 * consecutive rows of product t (0: M * x, 1: M^T * x) -- 1.0 on a matrix without structure, lower when neighbouring
 * rows share columns (the SpMV then walks per-XCD row ranges); *order_kind (may be NULL): 0 rows by smallest column,
 * 1 the file's order, 2 rows by the mean of their columns. */
int blz_locality(const blz_ctx *c, double locality[2], int *order_kind);

/* Read-only view of the plan of one slab (tests): what the launches of product `transpose` (0: M * x, 1: M^T * x), column
 * piece `piece` (0 unless the product is cut up for the exchange), WILL be -- taken from the same functions the launches
 * take their grids from.  Nothing is launched and nothing changes.  `plain` describes the product as blz_spmv and the
 * first product of an iteration run it, `dot` the same product with the inner products v^T Av, Av^T Av as its epilogue
 * (widths 1, 2, 4, 8; zero elsewhere); `fused` says whether blz_iterate uses `dot` for this piece. */
enum { BLZ_FORM_SPMV = 0, BLZ_FORM_STAGED = 1, BLZ_FORM_PANEL = 2 };
typedef struct blz_plan_launch {
	int32_t form;			/* BLZ_FORM_*: k_spmv / k_spmv_dot, k_spmv_staged, k_spmv_panel */
	int32_t xcd_ranges;		/* k_spmv / k_spmv_dot walk per-XCD row ranges: as applied, after the test on the grid size */
	int32_t split_log2;		/* k_spmv: 2^split_log2 lane groups share a row */
	int32_t st_gathers;		/* k_spmv_staged: gathers in flight per lane (4 / 8); 0 in the other forms */
	int64_t grid_stream;		/* workgroups of the streaming launch (256 threads; 1024 in the panel form) */
	int64_t grid_heavy;		/* ... of k_spmv_heavy (one per segment of a long row, bounded), 0: not launched */
	int64_t grid_combine;		/* ... of k_spmv_heavy_combine (one lane group per split row) */
	int64_t grid_medium;		/* ... of k_spmv_wave (one wavefront per medium row, 4 per workgroup) */
} blz_plan_launch;
typedef struct blz_plan {
	int64_t rows, cols, nnz;	/* of the piece */
	int32_t pieces;			/* column pieces of the product */
	int32_t width;			/* block width in HBM (the caller's n rounded up to a power of two unless BLZ_NO_PAD=1) */
	int32_t chunk;			/* products a dense sum takes between two reductions (make_modp) */
	int32_t num_cu;			/* compute units the grids are sized by */
	int32_t max_dot_blocks;		/* room for partial rows of the inner products */
	int32_t tail_batch;		/* k_spmv / k_spmv_dot instantiation: row tails as one predicated batch */
	int32_t xcd_ranges;		/* as planned (blz_plan_launch has it as applied) */
	uint32_t heavy_thr;		/* rows of MORE entries leave the streaming launch */
	int32_t n_medium, n_heavy, n_multi;	/* rows of k_spmv_wave, segments of k_spmv_heavy, split rows of the combine launch */
	int32_t st_ok, st_tr, st_pair, st_dyn, st_deep, st_interleave, st_capw, st_per_cu;	/* plan of the staged form */
	int32_t panel_rows;		/* block rows of the operand kept in LDS */
	int32_t packed;			/* values: 0 all ones, 1 packed palette, 2 separate array */
	int32_t dot_supported;		/* the width has the fused form at all */
	int32_t fused;			/* blz_iterate runs this piece as `dot` */
	int32_t fuse_local_off;		/* this matrix: inner products as their own kernel although the width could fuse */
	int32_t short_side;		/* the product runs in its short-side form: this describes that slab, piece 0 only */
	double locality;		/* lines of the operand per gathered entry (1: no reuse) */
	blz_plan_launch plain, dot;
} blz_plan;
int blz_slab_plan(const blz_ctx *c, int transpose, int piece, blz_plan *out);

/* Read-only view of the plan of one device block algebra call (tests): which kernels blz_dot_device, blz_dot_pair_device,
 * blz_combine_device or blz_combine_pair_device WILL run for `rows` rows (and `nterms` terms of a recombination; 1 for an
 * inner product) on blocks that all have a 16-byte aligned base and an even ld (aligned16 != 0) or not -- taken from the same
 * function the launches decide with.  Nothing is launched, nothing changes and no matrix is needed.  An op that is none of the
 * four, or nterms outside 1..BLZ_MAX_TERMS, is BLZ_EINVAL.  (The structure has the function's name: write `struct`.) */
enum { BLZ_DEVOP_DOT = 0, BLZ_DEVOP_DOT_PAIR = 1, BLZ_DEVOP_COMBINE = 2, BLZ_DEVOP_COMBINE_PAIR = 3 };
struct blz_devalg_plan {
	int32_t form;			/* 0: the vector-ALU kernels; 1: the matrix cores (p = 2^61 - 1, n = 8 or 16 only) */
	int32_t tile_rows;		/* form 1: rows of one MFMA tile (16 in a recombination, 64 in an inner product) */
	int32_t wavefronts;		/* form 1: wavefronts the launch starts; they take the tiles in turn */
	int32_t fold_tiles;		/* form 1, inner products: tiles between two folds of the int32 accumulators; else 0 */
	int64_t min_rows;		/* the threshold in force for this call kind and width (INT64_MAX: never by default) */
	int64_t lds_bytes;		/* form 1: LDS of a workgroup (a recombination: the coefficients' digit image) */
};
int blz_devalg_plan(const blz_ctx *c, int op, int64_t rows, int nterms, int aligned16, struct blz_devalg_plan *out);

/* The solver's numbering of one side (tests): perm[r] = the new index of original row r of `block`'s side, blz_rows(ctx, block)
 * words.  Returns 1 when a numbering is resident and 0 when it is the identity (perm is then 0, 1, 2, ...); a negative error
 * code for a bad argument or a context that holds one rank of several.  Host-built and device-built matrices alike. */
int blz_numbering(const blz_ctx *c, int block, int32_t *perm);

/* Short-side exchange: 1 when product `transpose` (0: M * x, 1: M^T * x) runs in its short-side form on this context
 * -- several ranks, 64-bit words, operand side at least 8 times longer than the output side (BLZ_SHORT_SIDE=0/1
 * overrides): the rank multiplies the transpose of its own rows of the other orientation by its own slab and a
 * reduce-scatter of the partial products replaces the all-gather of the long block.  In external-exchange mode
 * blz_spmv leaves the partial product on the device and blz_get_partial returns it (rows of the output side x n words,
 * original numbering, unreduced sums) for the caller to sum over the ranks. */
int blz_short_side(const blz_ctx *c, int transpose);
int blz_get_partial(blz_ctx *c, int transpose, uint64_t *host);

int64_t blz_rows(const blz_ctx *ctx, int block);	/* global row count of a block (N or C) */
/* size of this rank's slab of a block; *first = its first row in the SOLVER's numbering (see blz_owner_of_row) */
int64_t blz_local_rows(const blz_ctx *ctx, int block, int64_t *first);
int64_t blz_local_nnz(const blz_ctx *ctx, int transpose);		/* entries of this rank's slab of M (0) or M^T (1) */
int64_t blz_matrix_stream_bytes(const blz_ctx *ctx, int transpose);	/* bytes of that slab as resident in HBM
									 * (row_ptr + packed or plain col_idx/val) */

/* v <- random64() % p for this rank's rows, everything else 0 (:617-625). */
int blz_init_v(blz_ctx *ctx);

/* Copy a whole block (global rows x n, original row numbering) host->device / device->host.  With
 * nranks > 1 set_block fills the whole padded layout (so it doubles as an emulated all-gather); get_block
 * writes only the rows this rank owns and leaves the rest of `host` untouched.
 * The words given to set_block must be residues below p; they are not validated.  Every kernel writes canonical words,
 * so the blocks of an iteration are.  The products of a slab with wide entries (blz_slab_wide) rely on it: their x' = 2^32 x
 * mod p is a rotation of the 61-bit word at p = 2^61 - 1 and a Barrett reduction of 2^32 x < 2^94 otherwise. */
int blz_set_block(blz_ctx *ctx, int block, const uint64_t *host);
int blz_get_block(blz_ctx *ctx, int block, uint64_t *host);
int blz_set_small(blz_ctx *ctx, int which, const uint64_t *host);
int blz_get_small(blz_ctx *ctx, int which, uint64_t *host);

/* Device blocks: the same blocks handed over and taken back as DEVICE pointers -- a torch tensor, the output of the caller's
 * own kernel, the next vector of a Krylov method built on the operator -- without a trip through the host.  `dev` is
 * blz_rows(ctx, block) x n words of uint64_t in the ORIGINAL row numbering (border rows count on a bordered context), row-major
 * with a row stride of ld >= n words; words n .. ld-1 of a row are never read and never written.  The renumbering, the padded
 * width and the word width in HBM stay hidden, as for host blocks: one kernel gathers / scatters whole rows (DESIGN.md
 * section 15).  blz_set_block_device and blz_get_block_device mean what blz_set_block / blz_get_block mean (P explicit after
 * a set, materialised before a get); a blz_get_block after a device set, and a device get after blz_set_block, return the
 * same words.
 *   stream  the caller's hipStream_t (NULL = the null stream).  The call is ordered on it without synchronising the host: the
 *           library's stream waits for what the caller has enqueued so far, and the caller's stream waits for what the call
 *           enqueues.  A stream that is capturing a graph is BLZ_EINVAL.  (The first call after a matrix is set uploads the
 *           numbering once, synchronously.)
 *   bad     NULL: the words are not validated; the contract is blz_set_block's, residues below p.  Not NULL: the import counts
 *           the words >= p, the call synchronises, stores the count in *bad and, when it is not 0, returns BLZ_EINVAL with the
 *           count in the message -- the block then holds the words as given (truncated to 32 bits where p < 2^32).  The
 *           products of a slab with wide entries (blz_slab_wide) rely on canonical words: validate what is not known to be.
 * Every device pointer is checked on the host before anything is enqueued: the whole range ((rows - 1) * ld + n) * 8 bytes
 * must lie inside one allocation of the context's device.  A host pointer, memory of another device, a range that runs past
 * its allocation and ld < n are BLZ_EINVAL, and the message names the argument.
 * One rank only: a context with nranks > 1, a communicator, a loopback group or BLZ_FORCE_COMM answers BLZ_EINVAL. */
int blz_set_block_device(blz_ctx *ctx, int block, const uint64_t *dev, int64_t ld, void *stream, int64_t *bad);
int blz_get_block_device(blz_ctx *ctx, int block, uint64_t *dev, int64_t ld, void *stream);

/* y = M * x (transpose = 0) or M^T * x on caller-owned device blocks, bit-identical to blz_set_block(src, x);
 * blz_spmv(transpose, src, dst); blz_get_block(dst) on every kind of context -- plain, signed, wide, and bordered (then the
 * bordered operator, as blz_spmv) -- but without touching the state of a solve: V, TMP, AV, P, the small operands, the
 * iteration count and the implicit-p state stay exactly as they were, and a context whose solve has stopped still applies.
 * blz_apply_rows gives the row counts of x and y (either pointer may be NULL).  x and y (pointers, strides, stream: as above)
 * must not overlap.  The product runs in two scratch slabs of the context's own, one per side, allocated on first use:
 * (rows of V + rows of TMP) x the width in HBM x blz_word_bytes bytes.  blz_apply_release frees them (after waiting for
 * the context's stream); so do the next matrix-setting call and blz_destroy.  One rank only, as above. */
int blz_apply_rows(const blz_ctx *ctx, int transpose, int64_t *x_rows, int64_t *y_rows);
int blz_apply_device(blz_ctx *ctx, int transpose, const uint64_t *x, int64_t ldx, uint64_t *y, int64_t ldy, void *stream);
int blz_apply_release(blz_ctx *ctx);

/* Device block algebra: the other two parts of a Krylov step -- an n x n block inner product and a row-local recombination --
 * on caller-owned device blocks, exact mod p (64 x 64 -> 128-bit products, which no torch dtype does).  n and p are the
 * context's; `rows` is the CALLER's, any rows >= 0, not tied to a matrix: both calls work on a context with no matrix set and
 * on one whose solve is running or has stopped, and touch nothing of a solve (V, TMP, AV, P, the small operands, the control
 * words, the iteration count, the implicit-p state and the scratch slabs of blz_apply_device stay as they are).  Both
 * operations are invariant under a permutation of the rows, so they run on the caller's rows, in the caller's numbering, at
 * the caller's stride: no import, no export, no scratch slab.
 *   blocks        rows x n words of uint64_t, row stride ld >= n words whatever blz_word_bytes is; words n .. ld-1 of a row
 *                 are never read and never written.
 *   c, a[t]       n x n words of uint64_t, row-major, contiguous, in device memory.  Results land in device memory: nothing is
 *                 copied to the host and the host does not synchronise.
 *   every word read (blocks and coefficients) is a residue below p -- blz_set_block's contract, NOT validated; every word
 *   written is the canonical residue of the exact integer sum.
 *   stream        as for blz_set_block_device: the two-event ordering on the context's stream; a capturing stream is BLZ_EINVAL.
 * Checked on the host before the first enqueue, BLZ_EINVAL with a message that names the argument: rows < 0, nterms outside
 * 1..BLZ_MAX_TERMS, ld < n, a NULL entry, a host pointer, a block, c or a[t] that does not lie inside one allocation of the
 * context's device, and the overlaps below.  One rank only, as the other device-block calls.
 *
 * blz_dot_device      C = X^T * Y mod p:  c[i*n + j] = sum_r x[r*ldx + i] * y[r*ldy + j],  0 <= i, j < n.  dot(v, Av) is the
 *                     reference's vtAv.  x == y is allowed (a Gram matrix); c must overlap neither.  rows == 0: c = 0.  The
 *                     partial sums go through a scratch buffer of the context's own (at most 8 MB, allocated on first use,
 *                     freed by blz_destroy), not the one of an iteration in flight.
 * blz_combine_device  Z = sum_{t < nterms} X_t * A_t mod p, row by row:
 *                     z[r*ldz + j] = sum_t sum_i x[t][r*ldx[t] + i] * a[t][i*n + j].  z may BE one or more of the x[t] -- the
 *                     same pointer and the same stride: the in-place form, exact; otherwise z must overlap no x[t].  z must
 *                     overlap no a[t].  rows == 0: z is not touched.
 * Matrix cores: at p = 2^61 - 1 with 8-byte words and n = 8 or 16 both calls run as exact integer contractions of base-256
 * digits on v_mfma_i32_16x16x64_i8 (csrc/blz_devmfma.hip) -- the same words -- when BLZ_NO_MFMA is not 1,
 * every tall block of the call has a 16-byte aligned base and an even ld, and rows reaches the threshold of the call kind and
 * width: blz_dot_device 65 536 rows at n = 8 and at n = 16, blz_combine_device 1 048 576 rows at n = 8 and 65 536 at n = 16
 * (one MI355X, profiles/device_mfma_cost.txt).  BLZ_DEV_MFMA_MIN_ROWS=k, read at blz_create, sets every threshold to k (0:
 * always).  Anything else runs the vector-ALU kernels as before.  blz_combine_device keeps the digit image of its
 * coefficients in a scratch of the context's own: 132 096 bytes (the largest image: two outputs, four terms, n = 16),
 * allocated on first use and freed by blz_destroy; the inner products add no scratch to the partial rows above.
 * blz_devalg_plan reports the decision.
 * Limits: one rank; residues are not validated. */
#define BLZ_MAX_TERMS 4
int blz_dot_device(blz_ctx *ctx, int64_t rows, const uint64_t *x, int64_t ldx, const uint64_t *y, int64_t ldy, uint64_t *c,
		   void *stream);
int blz_combine_device(blz_ctx *ctx, int64_t rows, int nterms, const uint64_t *const *x, const int64_t *ldx,
		       const uint64_t *const *a, uint64_t *z, int64_t ldz, void *stream);

/* Device small algebra: the FOURTH part of a Krylov step -- the n x n algebra between the inner product and the recombination
 * -- and the echelon form of a caller's block, with the conventions of the device block algebra above: n and p are the
 * context's (n the caller's width), every operand is uint64_t words in device memory whatever blz_word_bytes is, n x n
 * operands are row-major and contiguous, results stay in device memory, the two-event ordering on `stream` with no host
 * synchronisation, a capturing stream is BLZ_EINVAL, one rank only, residues are NOT validated (blz_set_block's contract).
 * Each call works on a context with no matrix set, while a solve runs and after it has stopped, and touches nothing of a
 * solve: V, TMP, AV, P, the small operands, the control words (stop flag, npiv), the iteration count, the implicit-p state,
 * the scratch of blz_apply_device and blz_dot_device and the buffers of blz_block_rref / blz_kernel_basis stay as they are --
 * which is why blz_semi_inverse, which works on the context's own small operands and control words, cannot stand in.
 * Checked on the host before the first enqueue, BLZ_EINVAL with a message that names the argument: a NULL or host pointer, an
 * operand that does not lie inside one allocation of the context's device, rows < 0, ldx < n, and ANY overlap of an output
 * with an input or with another output (inputs may overlap each other).  Nothing is launched then.  DESIGN.md section 17.
 *
 * blz_semi_inverse_device   semi_inverse(), sequential/lanczos_modp.c:342-438, on the caller's n x n matrix vtav: writes winv
 *                           (n x n), d (n words, 0 or 1) and, unless it is NULL, npiv (ONE word: the pivot count).  Word for
 *                           word what blz_semi_inverse gives: the same pivot order, hence the same d and winv.  npiv = 0
 *                           comes with winv = 0 and d = 0, which is what the reference's two sweeps leave.  One launch.
 * blz_ortho_coeffs_device   the same semi-inverse AND the coefficients of orthogonalize(), :456-475, in ONE launch.  coef
 *                           receives BLZ_COEF_PANELS contiguous n x n panels of canonical residues; with D = diag(d),
 *                           W = winv and S = vtaav's column j where d[j] = 1, vtav's where d[j] = 0 (`spliced`, :462-466):
 *                               BLZ_COEF_V_AV  D                    BLZ_COEF_P_P  I - D
 *                               BLZ_COEF_V_V   (I - D) - W * S      BLZ_COEF_P_V  W
 *                               BLZ_COEF_V_P   -vtav * D
 *                           so that the row update of :478-491 is exactly
 *                               v' = combine(Av * coef[V_AV] + v * coef[V_V] + p * coef[V_P])
 *                               p' = combine(p * coef[P_P] + v * coef[P_V])
 *                           With npiv = 0 the panels are 0, I, 0, I, 0: the step is the identity on v and p, so a loop that
 *                           runs past the stop of :644-650 changes nothing and needs no look from the host to be safe.
 *                           npiv as above (may be NULL).
 * blz_rref_device           the canonical reduced row echelon form of the row space of the caller's block x: rows x n words,
 *                           row stride ldx >= n (the words past n of a row are never read), any rows >= 0.  No reference
 *                           counterpart; it is blz_block_rref and step 2 of blz_kernel_basis below on a caller's block.
 *                             e     n x n: rows sorted by pivot column, zero from the rank on -- the words blz_block_rref
 *                                   returns for the same rows
 *                             info  n + 1 int64_t words in DEVICE memory: info[0] = the rank, info[1 + i] = the pivot column
 *                                   of row i, -1 from the rank on
 *                             z     n x n, may be NULL: the canonical null basis of e -- one column per free column f,
 *                                   ascending, with 1 at f, -e[i][f] at pivot info[1 + i], 0 elsewhere; the columns from
 *                                   n - rank on are zero; z = I when the rank is 0
 *                           rows == 0: e = 0, rank 0, every pivot -1, z = I.  A block of full rank is decided after one tile
 *                           per workgroup and is NOT read whole; a deficient one is read once.  The partial echelons go
 *                           through a stack of the call's own (at most 2 x CUs x n x n words, 16 MB at n = 64) and two
 *                           control words, allocated on first use and freed by blz_destroy.  A stride so large that
 *                           rows * ldx leaves 64-bit byte offsets is BLZ_EINVAL.  With blz_apply_device and
 *                           blz_combine_device the four steps of blz_kernel_basis can be done on caller-owned candidates.
 * Limits: one rank; no capturing stream; residues are not validated; vector-ALU kernels only. */
#define BLZ_COEF_PANELS 5
enum { BLZ_COEF_V_AV = 0, BLZ_COEF_V_V = 1, BLZ_COEF_V_P = 2, BLZ_COEF_P_P = 3, BLZ_COEF_P_V = 4 };
int blz_semi_inverse_device(blz_ctx *ctx, const uint64_t *vtav, uint64_t *winv, uint64_t *d, uint64_t *npiv, void *stream);
int blz_ortho_coeffs_device(blz_ctx *ctx, const uint64_t *vtav, const uint64_t *vtaav, uint64_t *coef, uint64_t *npiv,
			    void *stream);
int blz_rref_device(blz_ctx *ctx, int64_t rows, const uint64_t *x, int64_t ldx, uint64_t *e, uint64_t *z, int64_t *info,
		    void *stream);

/* Fused device calls: the same parts of a Krylov step in fewer calls and fewer passes over the tall blocks -- z = op2 (op1 x),
 * two inner products against one block, two recombinations of shared inputs.  Every convention is that of the calls above:
 * uint64_t words in device memory, the context's n and p, row stride ld >= n with the words past n never read or written, the
 * two-event ordering on `stream` with no host synchronisation, a capturing stream and anything but one rank are BLZ_EINVAL,
 * every pointer is checked on the host before the first enqueue and the message names the argument, residues are NOT
 * validated, nothing of a solve is read or written.  With them a host-free step of the iteration is FOUR calls --
 * apply_pair, dot_pair, ortho_coeffs, combine_pair -- where it was seven.
 *
 * blz_apply_pair_device    transpose_first = 0: y = M * x, z = M^T * y;  transpose_first = 1: y = M^T * x, z = M * y.  x and z
 *                          have the x_rows of blz_apply_rows(ctx, transpose_first), y its y_rows.  y == NULL: the intermediate
 *                          is not wanted, ldy is ignored, and it lives only in the scratch slab of its side, neither exported
 *                          nor imported; y != NULL: it is exported as well (one pass more).  z may BE x -- the same pointer and
 *                          the same stride: the in-place form; otherwise x, y and z overlap one another nowhere.  Needs a
 *                          matrix; on a bordered context both products are the bordered operator, signed and wide slabs run
 *                          as in blz_apply_device, whose two scratch slabs and control words it shares.  Word for word what two
 *                          blz_apply_device calls give.
 * blz_dot_pair_device      c[0] = X0^T * Y and c[1] = X1^T * Y mod p, two contiguous n x n panels (2 * n * n words) in ONE pass:
 *                          dot_pair(v, Av, Av) gives vtAv and vtAAv where blz_ortho_coeffs_device takes them, c and c + n*n.
 *                          Any of x0, x1 and y may be the same block (the same pointer and the same stride), which is then
 *                          read once; c must overlap none of them.  rows == 0: both panels are zero.  Both triangles of a Gram
 *                          panel are written.  The partial sums go through a scratch buffer of this call's own (twice that of
 *                          blz_dot_device at the most, allocated on first use, freed by blz_destroy).  At n > 32 and
 *                          p >= 2^32 other than 2^61 - 1 the call runs the kernel of blz_dot_device twice.
 * blz_combine_pair_device  Z0 = sum_t X_t * A0_t and Z1 = sum_t X_t * A1_t mod p, 1 <= nterms <= BLZ_MAX_TERMS, every row of
 *                          every X_t read ONCE.  a0[t] or a1[t] may be NULL: term t does not enter that output.  A term that
 *                          enters neither output and an output with no term are BLZ_EINVAL, named.  Each of z0 and z1 may BE
 *                          one of the x[t] (the same pointer and the same stride); otherwise an output overlaps no x[t].  z0 and
 *                          z1 overlap each other nowhere and neither overlaps a coefficient matrix.  rows == 0: nothing is
 *                          touched.  One launch at every width and panel count.  The update of :478-491 is one call: terms
 *                          (Av, coef[V_AV], NULL), (v, coef[V_V], coef[P_V]), (p, coef[V_P], coef[P_P]), z0 = v, z1 = p.
 * Matrix cores: blz_dot_pair_device and blz_combine_pair_device take the matrix-core forms under the conditions stated at
 * blz_combine_device (p = 2^61 - 1, n = 8 or 16, 16-byte aligned blocks of even ld, BLZ_NO_MFMA not 1): blz_dot_pair_device from
 * 65 536 rows at either width, blz_combine_pair_device from 262 144 rows at n = 8 and 65 536 at n = 16 (BLZ_DEV_MFMA_MIN_ROWS
 * overrides); at n = 8 the pair's outputs share one 16-column tile.  The scratch is that of the unpaired calls.
 * Limits: one rank; no capturing stream; residues are not validated. */
int blz_apply_pair_device(blz_ctx *ctx, int transpose_first, const uint64_t *x, int64_t ldx, uint64_t *y, int64_t ldy,
			  uint64_t *z, int64_t ldz, void *stream);
int blz_dot_pair_device(blz_ctx *ctx, int64_t rows, const uint64_t *x0, int64_t ldx0, const uint64_t *x1, int64_t ldx1,
			const uint64_t *y, int64_t ldy, uint64_t *c, void *stream);
int blz_combine_pair_device(blz_ctx *ctx, int64_t rows, int nterms, const uint64_t *const *x, const int64_t *ldx,
			    const uint64_t *const *a0, const uint64_t *const *a1, uint64_t *z0, int64_t ldz0, uint64_t *z1,
			    int64_t ldz1, void *stream);

/* Device blocks on several ranks.  Everything above from blz_set_block_device on says "one rank only",
 * and that stays the default.  blz_set_device_ranks(ctx, 1) opens the family to a context that holds one rank's share of the
 * matrix: a block of the family is then RANK-LOCAL -- blz_local_rows(ctx, block, NULL) rows x n words of uint64_t, row stride
 * ld >= n, local row q being row first + q of the solver's numbering, the order the rank's slab already has (on one rank: all
 * rows, in the solver's numbering).  No rank needs memory for a whole block, and no call permutes a row.
 *   blz_set_device_ranks  sticky; before or after the matrix and the communicator; accepted on any context, a plain single
 *                         rank included; launches nothing.  Every rank of a job must set it alike: the caller's duty.  With the
 *                         mode off every call is byte for byte what it was.  blz_device_ranks reads it back.
 *   blz_local_row_ids     ids[q] = the ORIGINAL row number of local row q, blz_local_rows of them.  A host call, no GPU.  Over the
 *                         ranks of a job the ids partition 0 .. blz_rows - 1, and blz_owner_of_row(ctx, block, ids[q]) is this
 *                         rank.  (Needs a matrix, not the mode.)
 *   blz_take_local_device local <- the rank's rows of `global`, a whole block: blz_rows x n words in the ORIGINAL numbering.
 *   blz_put_local_device  the rank's rows of `global` <- local; no other row of `global` is touched.  Neither touches a word
 *                         past n of any row, neither is collective; both need the mode on and a matrix; pointer checks, the
 *                         two-event ordering on `stream` and the refusal of a capturing stream are those of
 *                         blz_set_block_device; local and global must not overlap.  For tests, start vectors, assembling results.
 * What the calls above mean with the mode on:
 *   blz_set_block_device, blz_get_block_device   the rank's rows to and from its slab, identity order; `bad` counts this rank's
 *                         words and is not collective.
 *   blz_apply_rows        the LOCAL row counts of x and y.
 *   blz_apply_device, blz_apply_pair_device      COLLECTIVE: every rank calls, with its own rows of x, y (and the intermediate).
 *                         Import into the scratch slab, the product with the solver's own exchange in all its pieces, export of
 *                         the rank's rows.  The bordered operator on a context set with blz_set_rhs_ranks; signed slabs as on
 *                         one rank.
 *   blz_dot_device, blz_dot_pair_device          COLLECTIVE: c = the sum over all ranks of X^T Y mod p, the same canonical words
 *                         on every rank.  `rows` is each rank's own, may differ between ranks and may be 0.  No matrix is
 *                         needed: the ranks are the communicator's.  The rank's residues go into a send buffer of the call's own,
 *                         one all-reduce of n * n (2 * n * n) words, one kernel reduces the sums mod p into c.  nranks * p > 2^64
 *                         is BLZ_EINVAL before anything is enqueued (blz_set_matrix's rule: the sum must not wrap).  On a
 *                         context that is not exchanging -- a plain single rank -- there is no collective.
 *   blz_combine_device, blz_combine_pair_device, blz_semi_inverse_device, blz_ortho_coeffs_device   allowed, unchanged, NOT
 *                         collective: row-local or n x n; the coefficients agree across ranks because the dots do.
 *   blz_rref_device       BLZ_EINVAL on anything but a plain single rank: the echelon on ranks is not built.
 * Refused with the mode on, by name, before the first enqueue and before any rendezvous: external-exchange mode (and
 * blz_set_exchange_mode(ctx, 1) afterwards), a product whose short-side form is active (blz_short_side), a capturing stream,
 * and the strides, pointers and overlaps refused above.  Every one of these checks is a function of things all ranks share
 * (the mode, the matrix' shape and partition, the communicator's size, p, the caller's strides being alike), so either all
 * ranks pass or all refuse and nobody waits at a rendezvous alone.  An error past the checks inside a collective call marks a
 * loopback group broken: its peers return BLZ_ECOMM at once.
 * As before no call reads or writes V, TMP, AV, P, the small operands, the control words, the iteration count or the
 * implicit-p state; the gathered operands are scratch that every product of an exchanging context refills.  A solve that runs
 * between the calls is unaffected.  No run on more than one GPU exists for this (or any) part of the library: the ranks of
 * its tests are loopback ranks on one device. */
int blz_set_device_ranks(blz_ctx *ctx, int on);
int blz_device_ranks(const blz_ctx *ctx);
int blz_local_row_ids(const blz_ctx *ctx, int block, int64_t *ids);
int blz_take_local_device(blz_ctx *ctx, int block, const uint64_t *global, int64_t ldg, uint64_t *local, int64_t ldl, void *stream);
int blz_put_local_device(blz_ctx *ctx, int block, const uint64_t *local, int64_t ldl, uint64_t *global, int64_t ldg, void *stream);

/* 32-bit device blocks: the same family on a caller's blocks of uint32_t words, valid exactly on
 * contexts with blz_word_bytes(ctx) == 4, i.e. p < 2^32 -- the reference's whole domain, and the width the solver's own slabs
 * have there.  Nothing above changes; the calls of the two families interleave freely on one context.
 *
 *   blocks        rows x n words of uint32_t, every ld counted in 32-bit words, ld >= n; words n .. ld-1 of a row are never
 *                 read or written.  A word is an UNSIGNED 32-bit residue: one that is >= 2^31 (common at p = 2^32 - 5) is not
 *                 negative, whatever the dtype of the tensor that holds it.  Pointers are aligned to 4 bytes; 8- and 16-byte
 *                 lane accesses are used where the pointer, the stride and n all allow them.
 *   c, a[t]       the n x n operands stay contiguous uint64_t words in device memory -- the results of blz_dot_device32 /
 *                 blz_dot_pair_device32, the coefficients of blz_combine_device32 / blz_combine_pair_device32 -- so
 *                 blz_ortho_coeffs_device and blz_semi_inverse_device serve both families unchanged.
 *   contract      each call writes exactly the words its 64-bit namesake writes when given the same residues zero-extended,
 *                 truncated to 32 bits.  Ordering on `stream`, the in-place forms, the overlaps refused, a NULL y of the
 *                 paired product, NULL coefficients of the paired recombination and rows == 0 are the namesake's.  `bad` of
 *                 blz_set_block_device32 counts the words >= p.
 *   scratch       the namesakes': the two slabs of blz_apply_device (blz_apply_release frees them) and the partial sums of
 *                 blz_dot_device / blz_dot_pair_device.  No buffer is added to a context.
 *   BLZ_EINVAL    on the host, before anything is enqueued, naming the argument: a context with p >= 2^32 ("residues do not fit
 *                 32-bit words"); a block pointer that is not aligned to 4 bytes; ld < n; a host pointer, or a range
 *                 ((rows - 1) * ld + n) * 4 bytes that does not lie inside one allocation of the context's device; a byte offset
 *                 that leaves 64 bits; the overlaps the namesakes refuse; a capturing stream; anything but a plain single rank
 *                 -- a communicator, a loopback group, BLZ_FORCE_COMM, or blz_set_device_ranks on.
 *   not built     there is no blz_rref_device32 and no blz_take_local_device32 / blz_put_local_device32: the echelon form
 *                 and device blocks on ranks take uint64_t blocks only. */
int blz_set_block_device32(blz_ctx *ctx, int block, const uint32_t *dev, int64_t ld, void *stream, int64_t *bad);
int blz_get_block_device32(blz_ctx *ctx, int block, uint32_t *dev, int64_t ld, void *stream);
int blz_apply_device32(blz_ctx *ctx, int transpose, const uint32_t *x, int64_t ldx, uint32_t *y, int64_t ldy, void *stream);
int blz_apply_pair_device32(blz_ctx *ctx, int transpose_first, const uint32_t *x, int64_t ldx, uint32_t *y, int64_t ldy,
			    uint32_t *z, int64_t ldz, void *stream);
int blz_dot_device32(blz_ctx *ctx, int64_t rows, const uint32_t *x, int64_t ldx, const uint32_t *y, int64_t ldy, uint64_t *c,
		     void *stream);
int blz_dot_pair_device32(blz_ctx *ctx, int64_t rows, const uint32_t *x0, int64_t ldx0, const uint32_t *x1, int64_t ldx1,
			  const uint32_t *y, int64_t ldy, uint64_t *c, void *stream);
int blz_combine_device32(blz_ctx *ctx, int64_t rows, int nterms, const uint32_t *const *x, const int64_t *ldx,
			 const uint64_t *const *a, uint32_t *z, int64_t ldz, void *stream);
int blz_combine_pair_device32(blz_ctx *ctx, int64_t rows, int nterms, const uint32_t *const *x, const int64_t *ldx,
			      const uint64_t *const *a0, const uint64_t *const *a1, uint32_t *z0, int64_t ldz0, uint32_t *z1,
			      int64_t ldz1, void *stream);

/* sparse_matrix_vector_product(y, M, x, transpose), sequential/lanczos_modp.c:266-287:
 * dst = M*src (transpose=0) or M^T*src (transpose=1), all n columns, canonical residues. */
int blz_spmv(blz_ctx *ctx, int transpose, int src_block, int dst_block);

/* block_dot_products(), :443-453: vtAv = v^T*Av, vtAAv = Av^T*Av (kept on the device;
 * copied to the host arrays when they are not NULL).  With nranks > 1 the partial products are
 * summed over ranks (RCCL all-reduce of 2*n*n words). */
int blz_block_dot(blz_ctx *ctx, uint64_t *vtAv, uint64_t *vtAAv);

/* semi_inverse(vtAv, winv, d), :342-438, on the device copy of vtAv (set it with blz_set_small
 * or blz_block_dot).  Same pivot order, hence the same d and winv. */
int blz_semi_inverse(blz_ctx *ctx, int *npiv, uint64_t *winv, uint64_t *d);

/* orthogonalize(), :456-492, followed by the copy v <- tmp of :655-656 (done in place). */
int blz_orthogonalize(blz_ctx *ctx);

/* The loop body of block_lanczos(), :631-659, up to max_iters times without host round trips.
 * *done = iterations completed (the reference's n_iterations increments), *stopped = 1 once
 * semi_inverse returned 0 (:644-650); later calls are then no-ops.  *ms (optional) = device time
 * of this call measured with HIP events on the context's stream. */
int blz_iterate(blz_ctx *ctx, int max_iters, int *done, int *stopped, float *ms);
int64_t blz_iterations(const blz_ctx *ctx);
/* Test hook, read-only: 1 while the iteration keeps p implicit (as X * E: the block v of the step before and an n x n
 * matrix on the device; blz_iterate on the matrix-core block update, unless BLZ_EXPLICIT_P=1 or BLZ_GRAPH=1), 0 when the
 * P block holds p itself.  Every call that looks at P (blz_get_block, blz_snapshot_begin, blz_orthogonalize, ...) makes
 * it explicit first; blz_set_block(P) makes it explicit. */
int blz_p_implicit(const blz_ctx *ctx);
/* Read-only: 1 when the next blz_iterate takes the self-dot path -- both inner products as products of a block with itself
 * (v^T Av = tmp^T tmp in the first product's kernel, v^T A^2 v = Av^T Av in the second's), v not read again -- and 0 when it
 * enqueues the step the other way.  The path needs: the fused second product (n in {1,2,4,8}, not BLZ_NO_FUSE=1), one rank
 * without collectives, no right-hand side, one piece per slab, both slabs in the streaming form without outlier rows, whole
 * rows per lane group in the first product, no BLZ_GRAPH=1, and not BLZ_NO_SELFDOT=1 (read when the context is created).
 * The results are the same words either way. */
int blz_selfdot_active(const blz_ctx *ctx);
int blz_set_iterations(blz_ctx *ctx, int64_t iterations);	/* --load-checkpoint */

/* final_check(), :560-582, on V and on TMP (= M^T v of the last iteration). */
int blz_final_check(blz_ctx *ctx, int *v_nonzero, int *vtm_zero);

/* Canonical reduced row echelon form of the row space of a block (any of the four; with several ranks every rank's rows,
 * merged through one all-gather of n x n words: collective, like blz_final_check).  rref = n x n words, row-major, rows
 * sorted by pivot column, rows from the rank on zero; *rank; pivots[i] = pivot column of row i, -1 from the rank on.  Any
 * output may be NULL.  The RREF is unique, so the words do not depend on the row order, the solver's renumbering, repeated
 * rows or the split over ranks.  A block of full rank is decided after one tile per workgroup (microseconds); a deficient
 * one is read once.  No reference counterpart; the nearest is final_check(), sequential/lanczos_modp.c:560-582. */
int blz_block_rref(blz_ctx *ctx, int block, uint64_t *rref, int *rank, int32_t *pivots);

/* Independent kernel vectors from the final block, in the state blz_iterate leaves on stop (TMP = the product of V):
 *   1. E1 = RREF(TMP), rank s, pivots P
 *   2. Z0 = the canonical null basis of E1: one column per free column f (not in P), ascending, with 1 at f, -E1[i][f] at
 *      pivot P[i], 0 elsewhere (Z0 = I when s = 0)
 *   3. Y = V Z0 (row by row, in place)
 *   4. E2 = RREF(Y): the basis is Y's columns at E2's pivots, k = rank(E2)
 * Leaves the basis in columns 0..k-1 of V and zeroes the others; z (n x n, may be NULL) gets the combination of the
 * original columns of V that gives each basis vector (column j; zero for j >= k).  Collective with several ranks. */
int blz_kernel_basis(blz_ctx *ctx, int *k, uint64_t *z);

/* The solution of a context with a right-hand side, in the state blz_iterate leaves on stop.  Runs blz_kernel_basis,
 * takes the first basis column whose border word is non-zero, scales it on the device so that the border word becomes
 * p - 1 (V keeps it in column 0, the other columns zero), recomputes the product of that column with the border applied
 * into TMP and checks on the GPU that it is zero (M x - b), then writes x (blz_rows(ctx, BLZ_V) - 1 words, original
 * numbering, the border row left out).  *status: 0 = solved and verified; 1 = no kernel vector with a non-zero border
 * word (an inconsistent system, or an unlucky start), x untouched; 2 = the verification failed (a bug), x untouched.
 * It is blz_solution_block on one right-hand side: the same status and the same V afterwards (zero where status is 1). */
int blz_solution(blz_ctx *ctx, uint64_t *x, int *status);

/* The solutions of a context with k = blz_rhs_count(ctx) right-hand sides (k == 1 included), in the same state.  Runs
 * blz_kernel_basis (kb vectors), solves W C = -I_k on the host for the k x kb border part W of the basis, and computes
 * V <- V C on the device: column i of V then is (y_i, -e_i) with M y_i = b_i, and zero where system i is not solvable
 * from this basis (e_i not in W's column space: an inconsistent system, or an unlucky start).  The side-1 product of V
 * with the border applied is recomputed into TMP and tested for zero on the GPU.  status[i]: 0 = solved and verified,
 * 1 = not solved (column i of x zero), 2 = the verification failed (a bug: every status is 2 and x is untouched).
 * x = (blz_rows(ctx, BLZ_V) - k) x k words, row-major, original numbering, the border rows left out.
 * blz_solution itself refuses a context with k > 1. */
int blz_solution_block(blz_ctx *ctx, uint64_t *x, int *status);

/* Asynchronous snapshot of (v, p, iteration count) for checkpoints (openMP/lanczos_modp.c:1013-1022 stops its loop
 * for them).  blz_snapshot_begin, called between two blz_iterate calls, enqueues the device-to-host copies of this
 * rank's rows on a stream of their own and returns; the GPU pauses for the transfer only and the caller goes on
 * iterating.  blz_snapshot_wait blocks until the copies have landed and writes this rank's rows into v and p (whole
 * blocks of rows(V) x n words, original numbering; other ranks' rows untouched).  It may be called from ANOTHER host
 * thread (the checkpoint writer) while the owner is inside blz_iterate -- the one exception to one thread per handle
 * (the in-flight mark is an atomic: begin in the owner's thread sees a wait that finished in the writer's).
 * v == p == NULL drops the snapshot: a writer that has failed (memory, one rank's copy) must still collect from EVERY
 * context, or their next blz_snapshot_begin is refused.  One snapshot in flight per context.
 * While the iteration keeps p implicit (blz_p_implicit), blz_snapshot_begin first makes the P block p: one more pass
 * over that block on the compute stream (X <- X * E), after which it waits for that stream -- idle between two
 * blz_iterate calls -- and resets E with a small blocking copy, before the asynchronous part above. */
int blz_snapshot_begin(blz_ctx *c);
int blz_snapshot_wait(blz_ctx *c, uint64_t *v, uint64_t *p, int64_t *iterations);

/* Measurement: run one hot-path kernel `reps` times between two HIP events on the context's
 * stream and return the mean time.  which: 0 = first SpMV of an iteration (:635), 1 = second (:636, without
 * the fused block products), 2 = block_dot + finalize, 3 = orthogonalize (updates V and P in place: call
 * blz_init_v or blz_set_block afterwards if the blocks are to be used again). */
int blz_time_kernel(blz_ctx *ctx, int which, int reps, float *ms_mean);
int blz_sync(blz_ctx *ctx);

/* Per-kernel HIP-event spans inside blz_iterate (on the stream the kernels run on).  blz_profile(ctx,1)
 * clears and starts collecting, blz_profile(ctx,0) stops; blz_profile_read sums the spans collected so
 * far into 8 classes: 0 first SpMV, 1 second SpMV, 2 block_dot (+finalize), 3 semi_inverse,
 * 4 orthogonalize, 5 all-gather of v, 6 all-gather of tmp, 7 all-reduce of the n x n products (and, on a bordered
 * several-rank context, of the k x n border words; the border kernels count with the product they follow). */
#define BLZ_PROFILE_CLASSES 8
int blz_profile(blz_ctx *ctx, int enable);
int blz_profile_read(blz_ctx *ctx, double ms_sum[BLZ_PROFILE_CLASSES], int64_t launches[BLZ_PROFILE_CLASSES]);

/* Exchange mode of a multi-rank context: 0 (default) = the library issues the RCCL collectives itself
 * inside blz_iterate / blz_block_dot; 1 = external: collectives are skipped and the caller moves the
 * slabs between ranks with blz_get_block / blz_set_block / blz_get_small / blz_set_small (used by the
 * single-GPU emulation tests of the sharded schedule; blz_iterate is refused in this mode).  A context that carries a
 * right-hand side on several ranks (blz_set_rhs_ranks) refuses external = 1 with BLZ_EINVAL. */
int blz_set_exchange_mode(blz_ctx *ctx, int external);

/* Multi-GPU (one process per GPU).  id_bytes = ncclUniqueId from blz_comm_unique_id() on rank 0,
 * broadcast by the caller (bench.py uses torch.distributed for that and nothing else).  Call blz_comm_init before
 * blz_set_matrix.  Inside blz_iterate every product is pipelined against the exchange of its operand: the block is
 * all-gathered in K pieces on a second stream and the product runs piece by piece behind it (K = up to 4 pieces of
 * >= 2 MB per slab, or BLZ_AG_CHUNKS). */
int blz_comm_unique_id(void *id_out, size_t id_bytes);	/* needs id_bytes >= 128 */
int blz_comm_init(blz_ctx *ctx, const void *id, size_t id_bytes, int rank, int nranks);
/* What the communicator itself says (ncclCommCount / ncclCommUserRank), not what the caller passed in: -1, -1 when the
 * context has none.  bench.py prints it so that an N > 1 line proves N ranks really met inside RCCL
 * (the reference prints its MPI_Comm_size, mpi/lanczos_modp.c:1755-1757). */
int blz_comm_info(const blz_ctx *ctx, int *nranks_seen, int *rank_seen);
/* pieces the exchange of product `transpose`'s operand (and the product itself) is cut into; 0 in the short-side form,
 * where nothing is gathered */
/* Loopback communicator: the contexts of ONE process on ONE device, one host thread each, as the ranks of a job -- RCCL
 * refuses two ranks on one GPU, and every other part of the multi-rank path (slabs, gathered layouts, the piece pipeline on
 * two streams, the landing buffers of the collectives, what a batch does past the stop) is then the production code run
 * with real multi-rank sums on a one-GPU box.  Create one group, attach every context (instead of blz_comm_init), drive
 * each context from its own thread: the collectives inside blz_iterate / blz_final_check meet in the group (a rank that
 * does not arrive within 120 s fails all of them with BLZ_ECOMM).  Not a transport: nothing leaves the device. */
typedef struct blz_loop_group blz_loop_group;
int blz_loop_group_create(int nranks, blz_loop_group **out);	/* at most 16 ranks */
void blz_loop_group_destroy(blz_loop_group *g);			/* after every attached context has been destroyed */
int blz_comm_init_loopback(blz_ctx *ctx, blz_loop_group *g, int rank);

int blz_exchange_pieces(const blz_ctx *ctx, int transpose);
/* the number of pieces this context would have a matrix of that shape prepared in for nranks ranks (what blz_prepare_for
 * passes to blz_prepare): for callers that prepare a rank's share themselves (blz_prepare_rank) */
int blz_exchange_pieces_for(const blz_ctx *ctx, int64_t mrows, int64_t mcols, int64_t nnz, int nranks);

#ifdef __cplusplus
}
#endif
#endif
