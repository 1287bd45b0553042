/* blz_mm_load_wide and the wide checkers under AddressSanitizer + UBSan (CPU build): extreme values, malformed and
 * truncated files, error paths included.
 * Compiled and run by tests/test_host_wide.py:  host_sanitize_wide <golden dir> <scratch dir> */
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

#define COORD "%%MatrixMarket matrix coordinate integer general\n"
#define COORD_F "%%%%MatrixMarket matrix coordinate integer general\n"	/* the same inside a printf format */
#define ARRAY "%%MatrixMarket matrix array integer general\n"
#define ARRAY_F "%%%%MatrixMarket matrix array integer general\n"

static void write_text(const char *path, const char *text)
{
	FILE *f = fopen(path, "w");
	REQUIRE(f != NULL);
	fputs(text, f);
	fclose(f);
}

static void expect_load(const char *path, const char *text, uint64_t p, int want)
{
	blz_coo M;
	uint32_t *hi = (uint32_t *)(uintptr_t)1;
	write_text(path, text);
	const int rc = blz_mm_load_wide(path, p, &M, &hi);
	if (rc != want) {
		fprintf(stderr, "blz_mm_load_wide gave %d, not %d, on:\n%s\n(%s)\n", rc, want, text, blz_last_error());
		exit(2);
	}
	if (rc == BLZ_OK) {
		blz_coo_free(&M);
		blz_values_free(hi);
	} else {
		REQUIRE(hi == NULL || want == BLZ_EINVAL);
	}
}

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t p) { return (uint64_t)((unsigned __int128)a * b % p); }

int main(int argc, char **argv)
{
	if (argc < 3)
		return 1;
	char m[4096], a[4096], b[4096], text[4096];
	snprintf(m, sizeof m, "%s/m.mtx", argv[2]);
	snprintf(a, sizeof a, "%s/x.mtx", argv[2]);
	snprintf(b, sizeof b, "%s/b.mtx", argv[2]);

	const uint64_t primes[] = { 65537, 4294967291ull, 4294967311ull, (1ull << 61) - 1, (1ull << 61) - 31, 4611686018427387847ull };
	for (int q = 0; q < 6; q++) {
		const uint64_t p = primes[q];
		blz_coo M;
		uint32_t *hi = NULL;
		/* the loader: residues of extreme values, duplicates, an empty row and an empty column */
		snprintf(text, sizeof text, COORD_F "%%c\n3 3 9\n1 1 0\n1 1 -1\n1 2 4294967296\n2 1 %" PRIu64 "\n2 2 %" PRIu64 "\n"
			 "2 1 9223372036854775807\n2 2 -9223372036854775808\n1 2 -1099511627776\n1 1 +4294967295\n", p, p + 5);
		write_text(m, text);
		REQUIRE(blz_mm_load_wide(m, p, &M, &hi) == BLZ_OK && M.nrows == 3 && M.ncols == 3 && M.nnz == 9);
		const uint64_t want[9] = { 0, p - 1, 4294967296ull % p, 0, 5 % p, 9223372036854775807ull % p,
					   (p - (9223372036854775808ull % p)) % p, (p - (1099511627776ull % p)) % p, 4294967295ull % p };
		int any = 0;
		for (int k = 0; k < 9; k++) {
			const uint64_t got = M.x[k] | ((uint64_t)(hi ? hi[k] : 0) << 32);
			REQUIRE(got == want[k]);
			any |= (want[k] >> 32) != 0;
		}
		REQUIRE((hi != NULL) == (any != 0));
		REQUIRE(p >= (1ull << 32) || hi == NULL);
		blz_coo_free(&M);
		blz_values_free(hi);
		blz_values_free(NULL);

		/* outside int64: never a wrap */
		expect_load(m, COORD "1 1 1\n1 1 9223372036854775808\n", p, BLZ_EIO);
		expect_load(m, COORD "1 1 1\n1 1 -9223372036854775809\n", p, BLZ_EIO);
		expect_load(m, COORD "1 1 1\n1 1 18446744073709551616\n", p, BLZ_EIO);
		expect_load(m, COORD "1 1 1\n1 1 99999999999999999999\n", p, BLZ_EIO);
		expect_load(m, COORD "1 1 1\n1 1 -99999999999999999999999999999999999999\n", p, BLZ_EIO);
		/* malformed and truncated */
		expect_load(m, "", p, BLZ_EFORMAT);
		expect_load(m, COORD, p, BLZ_EIO);
		expect_load(m, COORD "2 2\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 2\n1 1 1\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 2\n1 1 1\n2 2", p, BLZ_EIO);
		expect_load(m, COORD "2 2 1\n1 1 -\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 1\n1 1 x\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 1\n3 1 1\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 1\n1 0 1\n", p, BLZ_EIO);
		expect_load(m, COORD "2 2 0\n", p, BLZ_OK);
		expect_load(m, ARRAY "2 2\n1\n2\n3\n4\n", p, BLZ_EFORMAT);
		REQUIRE(blz_mm_load_wide("/nonexistent/m.mtx", p, &M, &hi) == BLZ_EIO);
		REQUIRE(blz_mm_load_wide(NULL, p, &M, &hi) == BLZ_EINVAL && blz_mm_load_wide(m, p, NULL, &hi) == BLZ_EINVAL);
		REQUIRE(blz_mm_load_wide(m, p, &M, NULL) == BLZ_EINVAL && blz_mm_load_wide(m, 1ull << 62, &M, &hi) == BLZ_EINVAL);

		/* the checkers: M = [[p - 1, 2^32 mod p], [-2^40, 0]], x = (p - 1, 2) */
		const uint64_t t32 = 4294967296ull % p, m40 = (p - 1099511627776ull % p) % p;
		snprintf(text, sizeof text, COORD_F "2 2 4\n1 1 %" PRIu64 "\n1 2 4294967296\n2 1 -1099511627776\n2 2 0\n", p - 1);
		write_text(m, text);
		const uint64_t y0 = (mulmod(p - 1, p - 1, p) + mulmod(t32, 2, p)) % p, y1 = mulmod(m40, p - 1, p);
		int64_t row = -7;
		int col = -7;
		snprintf(text, sizeof text, ARRAY_F "2 1\n%" PRIu64 "\n2\n", p - 1);
		write_text(a, text);
		snprintf(text, sizeof text, ARRAY_F "2 1\n%" PRIu64 "\n%" PRIu64 "\n", y0, y1);
		write_text(b, text);
		REQUIRE(blz_check_solution_wide(m, b, a, p, 1, &row) == 0);
		snprintf(text, sizeof text, ARRAY_F "2 1\n%" PRIu64 "\n%" PRIu64 "\n", y0, (y1 + 1) % p);
		write_text(b, text);
		REQUIRE(blz_check_solution_wide(m, b, a, p, 1, &row) == 2 && row == 1);
		REQUIRE(blz_check_solution_wide(m, b, a, p, 1, NULL) == 2);
		/* x M = ((p-1)(p-1) + 2 (-2^40), (p-1) 2^32) */
		snprintf(text, sizeof text, ARRAY_F "2 1\n%" PRIu64 "\n%" PRIu64 "\n", (mulmod(p - 1, p - 1, p) + mulmod(m40, 2, p)) % p,
			 mulmod(p - 1, t32, p));
		write_text(b, text);
		REQUIRE(blz_check_solution_wide(m, b, a, p, 0, &row) == 0);
		REQUIRE(blz_check_solution_wide(m, b, "/nonexistent/x.mtx", p, 0, &row) == BLZ_EIO);
		REQUIRE(blz_check_solution_wide(m, NULL, a, p, 0, &row) == BLZ_EINVAL);
		REQUIRE(blz_check_solution_wide(m, b, a, 1ull << 62, 0, &row) == BLZ_EINVAL);

		/* the block form: three columns -- right, wrong in row 0, zero */
		int status[BLZ_MAX_RHS];
		int64_t bad[BLZ_MAX_RHS];
		snprintf(text, sizeof text, ARRAY_F "2 3\n%" PRIu64 "\n2\n%" PRIu64 "\n2\n0\n0\n", p - 1, p - 1);
		write_text(a, text);
		snprintf(text, sizeof text, ARRAY_F "2 3\n%" PRIu64 "\n%" PRIu64 "\n%" PRIu64 "\n%" PRIu64 "\n7\n7\n", y0, y1, (y0 + 1) % p, y1);
		write_text(b, text);
		REQUIRE(blz_check_solution_block_wide(m, b, a, p, 1, status, bad) == 3);
		REQUIRE(status[0] == 0 && status[1] == 2 && bad[1] == 0 && status[2] == 3);
		REQUIRE(blz_check_solution_block_wide(m, b, a, p, 1, NULL, bad) == BLZ_EINVAL);

		/* a kernel: M = [[1, p - 1], [2^32 mod p, -(2^32)]] has (1, 1) in its right kernel */
		write_text(m, COORD "2 2 4\n1 1 1\n1 2 -1\n2 1 4294967296\n2 2 -4294967296\n");
		write_text(a, ARRAY "2 2\n1\n1\n5\n5\n");
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, &row, &col) == 0);
		write_text(a, ARRAY "2 2\n1\n1\n5\n6\n");
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, &row, &col) == 2 && row == 0 && col == 1);
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, NULL, NULL) == 2);
		write_text(a, ARRAY "2 1\n0\n0\n");
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, &row, &col) == 1);
		write_text(a, ARRAY "2 1\n0\n");
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, &row, &col) == BLZ_EIO);
		REQUIRE(blz_check_kernel_wide(NULL, a, p, 1, &row, &col) == BLZ_EINVAL);
		REQUIRE(blz_check_kernel_wide(m, a, 1ull << 62, 1, &row, &col) == BLZ_EINVAL);
		write_text(m, COORD "2 2 1\n1 1 9223372036854775808\n");
		REQUIRE(blz_check_kernel_wide(m, a, p, 1, &row, &col) == BLZ_EIO);	/* the matrix is refused */
		REQUIRE(blz_check_solution_wide(m, b, a, p, 1, &row) == BLZ_EIO);
		REQUIRE(blz_check_solution_block_wide(m, b, a, p, 1, status, bad) == BLZ_EIO);
	}

	/* a file of 200000 entries and more (the size at which the other loaders go parallel), with wide entries throughout */
	{
		const uint64_t p = (1ull << 61) - 1;
		const long nz = 200003;
		FILE *f = fopen(m, "w");
		REQUIRE(f != NULL);
		fputs(COORD, f);
		fprintf(f, "500 400 %ld\n", nz);
		for (long k = 0; k < nz; k++)
			fprintf(f, "%ld %ld %lld\n", k % 500 + 1, k % 400 + 1, k & 1 ? -(long long)k * 4294967311ll : (long long)k * 4294967311ll);
		fclose(f);
		blz_coo M;
		uint32_t *hi = NULL;
		REQUIRE(blz_mm_load_wide(m, p, &M, &hi) == BLZ_OK && M.nnz == nz && hi != NULL);
		const uint64_t w3 = p - 3ull * 4294967311ull, w4 = 4ull * 4294967311ull;
		REQUIRE((M.x[3] | ((uint64_t)hi[3] << 32)) == w3 && (M.x[4] | ((uint64_t)hi[4] << 32)) == w4);
		blz_coo_free(&M);
		blz_values_free(hi);
	}
	printf("wide host code clean under ASan + UBSan\n");
	return 0;
}
