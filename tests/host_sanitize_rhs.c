/* blz_rhs_load and blz_check_solution under AddressSanitizer + UBSan (CPU build), error paths included.
 * Compiled and run by tests/test_host_rhs.py:  host_sanitize_rhs <golden dir> <scratch dir> */
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
		uint64_t out[4] = { 7, 7, 7, 7 };
		write_text(b, "%%MatrixMarket matrix array integer general\n%comment\n3 1\n-1\n 0\n+5\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_OK && out[0] == p - 1 && out[1] == 0 && out[2] == 5 && out[3] == 7);
		REQUIRE(blz_rhs_load(b, p, 4, out) == BLZ_EIO && blz_rhs_load(b, p, 2, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix array integer general\n3 2\n1\n2\n3\n4\n5\n6\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix array integer general\n3 1\n1\n2\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix array integer general\n3 1\n1\n2\n3\n4\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix array integer general\n3 1\n1\nx\n3\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EIO);
		/* 19 digits beyond a signed 64-bit integer are still entries: 10^19 - 1 and 2^63, both signs */
		write_text(b, "%%MatrixMarket matrix array integer general\n4 1\n9999999999999999999\n-9999999999999999999\n"
			      "9223372036854775808\n-9223372036854775808\n");
		REQUIRE(blz_rhs_load(b, p, 4, out) == BLZ_OK);
		REQUIRE(out[0] == 9999999999999999999ull % p && out[1] == (p - 9999999999999999999ull % p) % p);
		REQUIRE(out[2] == 9223372036854775808ull % p && out[3] == (p - 9223372036854775808ull % p) % p);
		write_text(b, "%%MatrixMarket matrix array integer general\n1 1\n99999999999999999999\n");
		REQUIRE(blz_rhs_load(b, p, 1, out) == BLZ_EIO);
		write_text(b, "%%MatrixMarket matrix coordinate integer general\n3 1 1\n1 1 1\n");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EFORMAT);
		write_text(b, "");
		REQUIRE(blz_rhs_load(b, p, 3, out) == BLZ_EIO);
		REQUIRE(blz_rhs_load("/nonexistent/b.mtx", p, 3, out) == BLZ_EIO && blz_rhs_load(NULL, p, 3, out) == BLZ_EINVAL);

		/* x = (1, 1, ..., 1): b = the row sums (right) / column sums (left) of the matrix as loaded */
		blz_coo M;
		REQUIRE(blz_mm_load(mpath, p, &M) == BLZ_OK);
		for (int right = 0; right < 2; right++) {
			const int64_t xlen = right ? M.ncols : M.nrows, blen = right ? M.nrows : M.ncols;
			uint64_t *x = calloc((size_t)xlen + 1, sizeof *x), *y = calloc((size_t)blen + 1, sizeof *y);
			REQUIRE(x && y);
			for (int64_t i = 0; i < xlen; i++)
				x[i] = 1;
			for (int64_t u = 0; u < M.nnz; u++) {
				const int64_t j = right ? M.i[u] : M.j[u];
				y[j] = (y[j] + M.x[u]) % p;
			}
			REQUIRE(blz_save_block(a, xlen, 1, x) == BLZ_OK);
			FILE *f = fopen(b, "w");
			REQUIRE(f != NULL);
			fprintf(f, "%%%%MatrixMarket matrix array integer general\n%lld 1\n", (long long)blen);
			for (int64_t j = 0; j < blen; j++)	/* every other word as the negative representative */
				if (j & 1)
					fprintf(f, "-%" PRIu64 "\n", (p - y[j]) % p);
				else
					fprintf(f, "%" PRIu64 "\n", y[j]);
			fclose(f);
			int64_t bad = -1;
			REQUIRE(blz_check_solution(mpath, b, a, p, right, &bad) == 0 && bad == -1);
			REQUIRE(blz_check_solution(mpath, b, a, p, right, NULL) == 0);
			REQUIRE(blz_check_solution(mpath, b, a, p, !right, &bad) < 0);	/* the lengths belong to the other orientation */
			REQUIRE(blz_check_solution(mpath, b, "/nonexistent/x.mtx", p, right, &bad) == BLZ_EIO);
			REQUIRE(blz_check_solution(NULL, b, a, p, right, &bad) == BLZ_EINVAL);
			free(x);
			free(y);
		}
		blz_coo_free(&M);
	}
	printf("rhs host code clean under ASan + UBSan\n");
	return 0;
}
