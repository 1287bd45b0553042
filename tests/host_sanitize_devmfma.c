/* The host arithmetic of the device block algebra on the matrix cores (csrc/blz_devmfma_plan.h: the dispatch decision, the
 * launch geometry, the image layout) driven over its whole domain under AddressSanitizer + UndefinedBehaviorSanitizer.
 * Stand-alone: no library, no GPU.  Built and run by tests/test_host_sanitize_devmfma.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "blz_devmfma_plan.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static dm_env env_of(int mfma, int word, int m61, int n, int cus, int64_t thr)
{
	dm_env e;
	memset(&e, 0, sizeof e);
	e.mfma = mfma;
	e.word_bytes = word;
	e.p_is_m61 = m61;
	e.n = n;
	e.num_cu = cus;
	for (int op = 0; op < DM_NOPS; op++)
		for (int w = 0; w < 2; w++)
			e.min_rows[op][w] = thr;
	return e;
}

int main(void)
{
	/* the start: the lower end of a digit sum is 0 at the longest K', the upper end fits 25 bits, an accumulator between two
	 * MFMAs fits int32 */
	CHECK(DM_KMAX == 512 && (int64_t)DM_START - (int64_t)DM_KMAX * 255 * 128 == 0);
	CHECK((int64_t)DM_SUM_MAX == (int64_t)DM_KMAX * 255 * 255 && DM_SUM_MAX < (1 << 25));
	CHECK((int64_t)DM_START + 2 * (int64_t)DM_KMAX * 128 * 128 < INT32_MAX);
	/* the fold interval of an inner product: 2^30 +- tiles * 8 * 64 * 128 * 128 stays inside [2^29, 3 * 2^29] */
	CHECK((int64_t)DM_DOT_FOLD_TILES * 8 * DM_DOT_TILE_ROWS * 128 * 128 <= (1ll << 29));
	CHECK(dm_image_bytes_max() == 132096);

	static const int64_t rows_set[] = { 0, 1, 15, 16, 17, 63, 64, 65, 4099, 1911130, 1ll << 31, 1ll << 40, INT64_MAX };
	static const int64_t thr_set[] = { 0, 1, 1000, DM_ROWS_OFF };
	static const int widths[] = { 1, 4, 8, 12, 16, 32, 64 };
	static const int cu_set[] = { 0, 1, 8, 256, 304 };
	long forms = 0, calls = 0;
	unsigned char *seen = malloc((size_t)dm_image_bytes_max());
	CHECK(seen);
	for (int mfma = 0; mfma < 2; mfma++)
	for (int word = 4; word <= 8; word += 4)
	for (int m61 = 0; m61 < 2; m61++)
	for (size_t wi = 0; wi < sizeof widths / sizeof *widths; wi++)
	for (size_t ci = 0; ci < sizeof cu_set / sizeof *cu_set; ci++)
	for (size_t ti = 0; ti < sizeof thr_set / sizeof *thr_set; ti++) {
		const int n = widths[wi];
		const dm_env e = env_of(mfma, word, m61, n, cu_set[ci], thr_set[ti]);
		for (int op = -1; op <= DM_NOPS; op++)
		for (int nterms = 0; nterms <= DM_MAX_TERMS + 1; nterms++)
		for (int al = 0; al < 2; al++)
		for (size_t ri = 0; ri < sizeof rows_set / sizeof *rows_set; ri++) {
			const int64_t rows = rows_set[ri];
			dm_plan p;
			memset(&p, 0x5A, sizeof p);
			const int rc = dm_decide(&e, op, rows, nterms, al, &p);
			calls++;
			if (op < 0 || op >= DM_NOPS || nterms < 1 || nterms > DM_MAX_TERMS) {
				CHECK(rc == -1 && p.form == 0x5A5A5A5A);	/* untouched */
				continue;
			}
			CHECK(rc == 0);
			const int shape = mfma && word == 8 && m61 && (n == 8 || n == 16);
			const int want = shape && al && rows >= 1 && rows >= thr_set[ti];
			CHECK(p.form == want);
			CHECK(p.min_rows == (shape ? thr_set[ti] : DM_ROWS_OFF));
			if (!p.form) {
				CHECK(p.tile_rows == 0 && p.wavefronts == 0 && p.fold_tiles == 0 && p.lds_bytes == 0 && p.blocks == 0);
				continue;
			}
			forms++;
			CHECK(p.blocks >= 1 && p.threads >= 64 && p.threads <= 1024 && p.threads % 64 == 0);
			CHECK(p.wavefronts == p.blocks * (p.threads / 64));
			CHECK(p.lds_bytes > 0 && p.lds_bytes <= DM_LDS_PER_CU);
			const int cus = cu_set[ci] > 0 ? cu_set[ci] : 1;
			if (op == DM_OP_DOT || op == DM_OP_DOT_PAIR) {
				CHECK(p.tile_rows == 64 && p.fold_tiles == 64 && p.threads == DM_DOT_THREADS && p.blocks <= 2 * cus);
				CHECK(p.lds_bytes == dm_dot_lds_bytes(op, n));
				/* no workgroup without a tile */
				CHECK((int64_t)(p.blocks - 1) * 4 < rows / 64 + (rows % 64 != 0));
			} else {
				CHECK(p.tile_rows == 16 && p.fold_tiles == 0);
				CHECK(p.sets == (op == DM_OP_COMBINE_PAIR && n == 16 ? 2 : 1) && p.ksteps * 8 == n * nterms);
				CHECK(p.image_bytes == p.lds_bytes && p.image_bytes <= dm_image_bytes_max());
				CHECK(p.ksteps * 64 <= DM_KMAX);
				CHECK((int64_t)p.blocks * (p.threads / 64) <= (int64_t)cus * DM_WAVES_PER_CU);
				CHECK((int64_t)(p.threads / 64) * (DM_LDS_PER_CU / p.lds_bytes) >= 1);
				/* the image: every fragment and every start inside it, none on another */
				memset(seen, 0, (size_t)p.image_bytes);
				for (int st = 0; st < p.sets; st++)
					for (int ks = 0; ks < p.ksteps; ks++)
						for (int dg = 0; dg < DM_ND; dg++)
							for (int lane = 0; lane < 64; lane++) {
								const int64_t at = dm_image_frag_at(p.ksteps, st, ks, dg, lane);
								CHECK(at >= 0 && at + 16 <= dm_image_b_bytes(p.sets, p.ksteps) && at % 16 == 0);
								for (int b = 0; b < 16; b++)
									CHECK(seen[at + b]++ == 0);
							}
				for (int st = 0; st < p.sets; st++)
					for (int dg = 0; dg < DM_ND; dg++)
						for (int col = 0; col < 16; col++) {
							const int64_t at = dm_image_init_at(p.sets, p.ksteps, st, dg, col);
							CHECK(at >= dm_image_b_bytes(p.sets, p.ksteps) && at + 4 <= p.image_bytes && at % 4 == 0);
							for (int b = 0; b < 4; b++)
								CHECK(seen[at + b]++ == 0);
						}
				for (int64_t b = 0; b < p.image_bytes; b++)
					CHECK(seen[b] == 1);
			}
		}
	}
	free(seen);
	/* the defaults: a threshold or "never", and never a 16-row call */
	for (int op = 0; op < DM_NOPS; op++)
		for (int n = 8; n <= 16; n += 8)
			CHECK(dm_default_min_rows(op, n) > 16);
	CHECK(forms > 1000);
	printf("dm_decide: %ld calls, %ld matrix-core plans: clean under ASan + UBSan\n", calls, forms);
	return 0;
}
