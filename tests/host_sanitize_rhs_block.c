/* blz_rhs_load_block and blz_check_solution_block under AddressSanitizer + UBSan (CPU build), error paths included.
 * Compiled and run by tests/test_host_rhs_block.py:  host_sanitize_rhs_block <golden dir> <scratch dir> */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "blz.h"

#define REQUIRE(cond)                                                                         \
	do {                                                                                  \
		if (!(cond)) {                                                                \
			fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, blz_last_error()); \
			exit(2);                                                              \
		}                                                                             \
	} while (0)

#define BANNER "%%MatrixMarket matrix array integer general\n"

static void write_text(const char *path, const char *text)
{
	FILE *f = fopen(path, "w");
	REQUIRE(f != NULL);
	fputs(text, f);
	fclose(f);
}

int main(int argc, char **argv)
{
	if (argc < 3)
		return 1;
	char mpath[4096], a[4096], b[4096];
	snprintf(mpath, sizeof mpath, "%s/quirks40x30.mtx", argv[1]);
	snprintf(a, sizeof a, "%s/x.mtx", argv[2]);
	snprintf(b, sizeof b, "%s/b.mtx", argv[2]);
	const uint64_t primes[] = { 65537, 2147483647ull, 4294967291ull, (1ull << 61) - 1 };
	for (int q = 0; q < 4; q++) {
		const uint64_t p = primes[q];
		uint64_t out[7] = { 7, 7, 7, 7, 7, 7, 7 };
		int k = -1;
		/* column-major in the file, row-major in memory, exactly len * k words written */
		write_text(b, BANNER "%comment\n3 2\n-1\n 0\n+5\n1\n2\n-3\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_OK && k == 2);
		REQUIRE(out[0] == p - 1 && out[1] == 1 && out[2] == 0 && out[3] == 2 && out[4] == 5 && out[5] == p - 3 && out[6] == 7);
		REQUIRE(blz_rhs_load_block(b, p, 3, 16, &k, NULL) == BLZ_OK && k == 2);	/* the size line only */
		REQUIRE(blz_rhs_load_block(b, p, -1, 16, &k, NULL) == BLZ_OK && k == 2);	/* any row count */
		REQUIRE(blz_rhs_load_block(b, p, 4, 2, &k, out) == BLZ_EIO && k == 0);
		REQUIRE(blz_rhs_load_block(b, p, 3, 1, &k, out) == BLZ_EIO && k == 2);		/* k > kmax: k is still reported */
		REQUIRE(blz_rhs_load_block(b, p, -1, 2, &k, out) == BLZ_EINVAL);
		REQUIRE(blz_rhs_load_block(b, p, 3, 0, &k, out) == BLZ_EINVAL && blz_rhs_load_block(b, p, 3, 2, NULL, out) == BLZ_EINVAL);
		write_text(b, BANNER "3 1\n4\n5\n6\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_OK && k == 1 && out[0] == 4 && out[2] == 6);
		write_text(b, BANNER "3 2\n1\n2\n3\n4\n5\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		write_text(b, BANNER "3 2\n1\n2\n3\n4\n5\n6\n7\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		write_text(b, BANNER "3 2\n1\n2\nx\n4\n5\n6\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		write_text(b, BANNER "3 0\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		write_text(b, BANNER "3 -2\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		write_text(b, BANNER "1 2\n99999999999999999999\n1\n");
		REQUIRE(blz_rhs_load_block(b, p, 1, 2, &k, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix coordinate integer general\n3 2 1\n1 1 1\n");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EFORMAT);
		write_text(b, "");
		REQUIRE(blz_rhs_load_block(b, p, 3, 2, &k, out) == BLZ_EIO);
		REQUIRE(blz_rhs_load_block("/nonexistent/b.mtx", p, 3, 2, &k, out) == BLZ_EIO);
		REQUIRE(blz_rhs_load_block(NULL, p, 3, 2, &k, out) == BLZ_EINVAL);

		/* x_t = (t + 1, ..., t + 1): b_t = (t + 1) * the row sums (right) / column sums (left); column 1 of x zero,
		 * column 2 with one word off */
		blz_coo M;
		REQUIRE(blz_mm_load(mpath, p, &M) == BLZ_OK);
		for (int right = 0; right < 2; right++) {
			const int64_t xlen = right ? M.ncols : M.nrows, blen = right ? M.nrows : M.ncols;
			const int kk = 4;
			uint64_t *x = calloc((size_t)(xlen * kk) + 1, sizeof *x), *y = calloc((size_t)blen + 1, sizeof *y);
			REQUIRE(x && y);
			for (int64_t i = 0; i < xlen; i++)
				for (int t = 0; t < kk; t++)
					x[i * kk + t] = t == 1 ? 0 : (uint64_t)(t + 1);
			int64_t used = -1;	/* a word of x that some entry of the matrix reads */
			for (int64_t u = 0; u < M.nnz; u++) {
				const int64_t j = right ? M.i[u] : M.j[u];
				y[j] = (y[j] + M.x[u]) % p;
				if (used < 0 && M.x[u])
					used = right ? M.j[u] : M.i[u];
			}
			REQUIRE(used >= 0);
			x[used * kk + 2] = 5;
			REQUIRE(blz_save_block(a, xlen, kk, x) == BLZ_OK);
			FILE *f = fopen(b, "w");
			REQUIRE(f != NULL);
			fputs(BANNER, f);
			fprintf(f, "%lld %d\n", (long long)blen, kk);
			for (int t = 0; t < kk; t++)
				for (int64_t j = 0; j < blen; j++) {	/* every other word as the negative representative */
					const uint64_t w = (uint64_t)((unsigned __int128)y[j] * (unsigned)(t + 1) % p);
					if (j & 1)
						fprintf(f, "-%" PRIu64 "\n", (p - w) % p);
					else
						fprintf(f, "%" PRIu64 "\n", w);
				}
			fclose(f);
			int status[BLZ_MAX_RHS];
			int64_t bad[BLZ_MAX_RHS];
			REQUIRE(blz_check_solution_block(mpath, b, a, p, right, status, bad) == kk);
			REQUIRE(status[0] == 0 && status[1] == 3 && status[2] == 2 && status[3] == 0 && bad[0] == -1 && bad[2] >= 0);
			REQUIRE(blz_check_solution_block(mpath, b, a, p, right, status, NULL) == kk && status[2] == 2);
			REQUIRE(blz_check_solution_block(mpath, b, a, p, !right, status, bad) < 0);	/* the other orientation's lengths */
			REQUIRE(blz_check_solution_block(mpath, b, "/nonexistent/x.mtx", p, right, status, bad) == BLZ_EIO);
			REQUIRE(blz_check_solution_block(NULL, b, a, p, right, status, bad) == BLZ_EINVAL);
			REQUIRE(blz_check_solution_block(mpath, b, a, p, right, NULL, bad) == BLZ_EINVAL);
			REQUIRE(blz_save_block(a, xlen, 1, x) == BLZ_OK);	/* a column count that differs from b's */
			REQUIRE(blz_check_solution_block(mpath, b, a, p, right, status, bad) == BLZ_EIO);
			free(x);
			free(y);
		}
		blz_coo_free(&M);
	}
	printf("rhs block host code clean under ASan + UBSan\n");
	return 0;
}
