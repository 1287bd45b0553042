/* blz_mm_load_signed and the signed checkers under AddressSanitizer + UBSan (CPU build): malformed, truncated and
 * extreme-value files, error paths included.
 * Compiled and run by tests/test_host_signed.py:  host_sanitize_signed <golden dir> <scratch dir> */
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
#define ARRAY "%%MatrixMarket matrix array integer general\n"
#define ARRAY_F "%%%%MatrixMarket matrix array integer general\n"	/* the same inside a printf format */

static void write_text(const char *path, const char *text)
{
	FILE *f = fopen(path, "w");
	REQUIRE(f != NULL);
	fputs(text, f);
	fclose(f);
}

static void expect_load(const char *path, const char *text, int want)
{
	blz_coo M;
	write_text(path, text);
	const int rc = blz_mm_load_signed(path, &M);
	if (rc != want) {
		fprintf(stderr, "blz_mm_load_signed gave %d, not %d, on:\n%s\n(%s)\n", rc, want, text, blz_last_error());
		exit(2);
	}
	if (rc == BLZ_OK)
		blz_coo_free(&M);
}

int main(int argc, char **argv)
{
	if (argc < 3)
		return 1;
	char m[4096], a[4096], b[4096], g[4096];
	snprintf(m, sizeof m, "%s/m.mtx", argv[2]);
	snprintf(a, sizeof a, "%s/x.mtx", argv[2]);
	snprintf(b, sizeof b, "%s/b.mtx", argv[2]);
	snprintf(g, sizeof g, "%s/quirks40x30.mtx", argv[1]);

	/* the loader: extreme values as bit patterns */
	blz_coo M;
	write_text(m, COORD "%c\n2 3 5\n1 1 -1\n2 3 -2147483648\n1 2 2147483647\n2 1 0\n2 2 +5\n");
	REQUIRE(blz_mm_load_signed(m, &M) == BLZ_OK && M.nrows == 2 && M.ncols == 3 && M.nnz == 5);
	REQUIRE(M.x[0] == 0xFFFFFFFFu && M.x[1] == 0x80000000u && M.x[2] == 0x7FFFFFFFu && M.x[3] == 0 && M.x[4] == 5);
	REQUIRE(M.i[1] == 1 && M.j[1] == 2);
	blz_coo_free(&M);
	/* the golden file with the reference's quirks loads in both modes; its words differ only where an entry is negative */
	{
		blz_coo U;
		REQUIRE(blz_mm_load_signed(g, &M) == BLZ_OK && blz_mm_load(g, (1ull << 61) - 1, &U) == BLZ_OK && U.nnz == M.nnz);
		REQUIRE(memcmp(U.x, M.x, sizeof *U.x * (size_t)U.nnz) == 0);	/* p >= 2^32: the same words */
		blz_coo_free(&U);
		blz_coo_free(&M);
	}
	/* outside int32, also through a wrapped 64-bit accumulator */
	expect_load(m, COORD "1 1 1\n1 1 2147483648\n", BLZ_EIO);
	expect_load(m, COORD "1 1 1\n1 1 -2147483649\n", BLZ_EIO);
	expect_load(m, COORD "1 1 1\n1 1 18446744073709551616\n", BLZ_EIO);
	expect_load(m, COORD "1 1 1\n1 1 -18446744073709551617\n", BLZ_EIO);
	expect_load(m, COORD "1 1 1\n1 1 99999999999999999999999999999999999999\n", BLZ_EIO);
	/* malformed and truncated */
	expect_load(m, "", BLZ_EFORMAT);
	expect_load(m, COORD, BLZ_EIO);
	expect_load(m, COORD "2 2\n", BLZ_EIO);
	expect_load(m, COORD "2 2 2\n1 1 1\n", BLZ_EIO);
	expect_load(m, COORD "2 2 2\n1 1 1\n2 2", BLZ_EIO);
	expect_load(m, COORD "2 2 1\n1 1 -\n", BLZ_EIO);
	expect_load(m, COORD "2 2 1\n1 1 x\n", BLZ_EIO);
	expect_load(m, COORD "2 2 1\n3 1 1\n", BLZ_EIO);
	expect_load(m, COORD "2 2 1\n1 0 1\n", BLZ_EIO);
	expect_load(m, COORD "-2 2 1\n1 1 1\n", BLZ_EIO);
	expect_load(m, COORD "2 2 0\n", BLZ_OK);
	expect_load(m, ARRAY "2 2\n1\n2\n3\n4\n", BLZ_EFORMAT);
	expect_load(m, "%%MatrixMarket matrix coordinate real general\n1 1 1\n1 1 1\n", BLZ_EFORMAT);
	REQUIRE(blz_mm_load_signed("/nonexistent/m.mtx", &M) == BLZ_EIO);
	REQUIRE(blz_mm_load_signed(NULL, &M) == BLZ_EINVAL && blz_mm_load_signed(m, NULL) == BLZ_EINVAL);

	/* a file large enough for the parallel reader (200000 entries and more), good and with one entry out of range */
	{
		const long nz = 200003;
		FILE *f = fopen(m, "w");
		REQUIRE(f != NULL);
		fputs(COORD, f);
		fprintf(f, "500 400 %ld\n", nz);
		for (long k = 0; k < nz; k++)
			fprintf(f, "%ld %ld %ld\n", k % 500 + 1, k % 400 + 1, k == nz - 2 ? -2147483648l : (k & 1 ? -(k % 9) : k % 9));
		fclose(f);
		REQUIRE(blz_mm_load_signed(m, &M) == BLZ_OK && M.nnz == nz && M.x[nz - 2] == 0x80000000u && M.x[3] == (uint32_t)-3);
		blz_coo_free(&M);
		f = fopen(m, "w");
		REQUIRE(f != NULL);
		fputs(COORD, f);
		fprintf(f, "500 400 %ld\n", nz);
		for (long k = 0; k < nz; k++)
			fprintf(f, "%ld %ld %s\n", k % 500 + 1, k % 400 + 1, k == nz - 2 ? "2147483648" : "-1");
		fclose(f);
		REQUIRE(blz_mm_load_signed(m, &M) == BLZ_EIO);
	}

	/* the checkers on a path graph's incidence matrix: 3 edges x 4 vertices, rows (+1, -1); one entry written as
	 * INT32_MIN and one as INT32_MAX in a second matrix */
	const uint64_t primes[] = { 65537, 2147483647ull, 4294967291ull, (1ull << 61) - 1, 4611686018427387847ull };
	for (int q = 0; q < 5; q++) {
		const uint64_t p = primes[q];
		int64_t row = -7;
		int col = -7;
		write_text(m, COORD "3 4 6\n1 1 1\n1 2 -1\n2 2 1\n2 3 -1\n3 3 1\n3 4 -1\n");
		write_text(a, ARRAY "4 2\n1\n1\n1\n1\n5\n5\n5\n5\n");
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == 0);
		REQUIRE(blz_check_kernel(m, a, p, 1, &row, &col) == 2 && row == 0 && col == 0);	/* -1 as 2^32 - 1: another matrix */
		write_text(a, ARRAY "4 2\n1\n1\n1\n1\n5\n5\n6\n5\n");
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == 2 && row == 1 && col == 1);
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, NULL, NULL) == 2);
		write_text(a, ARRAY "4 1\n0\n0\n0\n0\n");
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == 1);
		REQUIRE(blz_check_kernel_signed(m, a, p, 0, &row, &col) == BLZ_EINVAL);	/* 4 rows, the left kernel has 3 */
		write_text(a, ARRAY "4 1\n0\n0\n");
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == BLZ_EIO);
		char big[256];
		snprintf(big, sizeof big, ARRAY_F "4 1\n1\n1\n1\n%" PRIu64 "\n", p);
		write_text(a, big);
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == BLZ_EINVAL);
		REQUIRE(blz_check_kernel_signed(NULL, a, p, 1, &row, &col) == BLZ_EINVAL);
		REQUIRE(blz_check_kernel_signed(m, a, 1ull << 62, 1, &row, &col) == BLZ_EINVAL);
		REQUIRE(blz_check_kernel_signed("/nonexistent/m.mtx", a, p, 1, &row, &col) == BLZ_EIO);

		/* M = [[INT32_MIN, INT32_MAX], [-1, 0]], x = (p - 1, 2): M x = (2^31 + 2 (2^31 - 1), 1) = (3 * 2^31 - 2, 1) mod p */
		write_text(m, COORD "2 2 4\n1 1 -2147483648\n1 2 2147483647\n2 1 -1\n2 2 0\n");
		char xs[256], bs[256];
		snprintf(xs, sizeof xs, ARRAY_F "2 1\n%" PRIu64 "\n2\n", p - 1);
		write_text(a, xs);
		snprintf(bs, sizeof bs, ARRAY_F "2 1\n%" PRIu64 "\n1\n", (uint64_t)((3ull * 2147483648ull - 2ull) % p));
		write_text(b, bs);
		REQUIRE(blz_check_solution_signed(m, b, a, p, 1, &row) == 0);
		snprintf(bs, sizeof bs, ARRAY_F "2 1\n%" PRIu64 "\n-%" PRIu64 "\n", (uint64_t)((3ull * 2147483648ull - 2ull) % p), p - 1);
		write_text(b, bs);
		REQUIRE(blz_check_solution_signed(m, b, a, p, 1, &row) == 0);		/* b's -(p - 1) is 1 */
		snprintf(bs, sizeof bs, ARRAY_F "2 1\n%" PRIu64 "\n2\n", (uint64_t)((3ull * 2147483648ull - 2ull) % p));
		write_text(b, bs);
		REQUIRE(blz_check_solution_signed(m, b, a, p, 1, &row) == 2 && row == 1);
		REQUIRE(blz_check_solution_signed(m, b, a, p, 1, NULL) == 2);
		/* x M with x = (p - 1, 2): (2^31 - 2, -(2^31 - 1)) mod p */
		snprintf(bs, sizeof bs, ARRAY_F "2 1\n%" PRIu64 "\n-2147483647\n", (uint64_t)((2147483648ull - 2ull) % p));
		write_text(b, bs);
		REQUIRE(blz_check_solution_signed(m, b, a, p, 0, &row) == 0);
		REQUIRE(blz_check_solution_signed(m, b, "/nonexistent/x.mtx", p, 0, &row) == BLZ_EIO);
		REQUIRE(blz_check_solution_signed(m, NULL, a, p, 0, &row) == BLZ_EINVAL);
		write_text(b, ARRAY "3 1\n1\n2\n3\n");
		REQUIRE(blz_check_solution_signed(m, b, a, p, 0, &row) == BLZ_EIO);

		/* the block form: three columns -- right, wrong in row 0, zero */
		int status[BLZ_MAX_RHS];
		int64_t bad[BLZ_MAX_RHS];
		snprintf(xs, sizeof xs, ARRAY_F "2 3\n%" PRIu64 "\n2\n%" PRIu64 "\n2\n0\n0\n", p - 1, p - 1);
		write_text(a, xs);
		const uint64_t y0 = (3ull * 2147483648ull - 2ull) % p;
		snprintf(bs, sizeof bs, ARRAY_F "2 3\n%" PRIu64 "\n1\n%" PRIu64 "\n1\n7\n7\n", y0, (y0 + 1) % p);
		write_text(b, bs);
		REQUIRE(blz_check_solution_block_signed(m, b, a, p, 1, status, bad) == 3);
		REQUIRE(status[0] == 0 && status[1] == 2 && bad[1] == 0 && status[2] == 3 && bad[0] == -1);
		REQUIRE(blz_check_solution_block_signed(m, b, a, p, 1, status, NULL) == 3 && status[1] == 2);
		REQUIRE(blz_check_solution_block_signed(m, b, a, p, 1, NULL, bad) == BLZ_EINVAL);
		write_text(a, ARRAY "2 2\n1\n2\n3\n4\n");
		REQUIRE(blz_check_solution_block_signed(m, b, a, p, 1, status, bad) == BLZ_EIO);	/* 2 columns of x for 3 of b */
		write_text(m, COORD "2 2 1\n1 1 4294967295\n");
		REQUIRE(blz_check_solution_block_signed(m, b, a, p, 1, status, bad) == BLZ_EIO);	/* the matrix is refused */
		REQUIRE(blz_check_solution_signed(m, b, a, p, 1, &row) == BLZ_EIO);
		REQUIRE(blz_check_kernel_signed(m, a, p, 1, &row, &col) == BLZ_EIO);
	}
	printf("signed host code clean under ASan + UBSan\n");
	return 0;
}
