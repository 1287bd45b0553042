/*
 * checker_modp -- drop-in for the reference's verifier (checker_modp.c) with residues widened to 64 bits, so
 * that kernels computed modulo primes above 2^31-1 can be checked too.  Same flags (:43-76), same verdict
 * lines and exit codes: "OK" + exit 0, or a KO message + exit 1.  Plain C, no GPU.
 * --independent (no reference counterpart) also asks that the kernel vectors be linearly independent mod P.
 * --rhs FILE (no reference counterpart) checks a solution instead: --kernel names the file of x, and M*x == b (--right)
 * or x*M == b (--left) is asked for the vector b of FILE.  With k > 1 columns in FILE, --kernel holds the k columns of x and
 * each is checked against its own b; an all-zero column of x stands for a system that was not solved and does not fail.
 * --signed (no reference counterpart) reads the matrix in signed value mode: an entry a (an int32) means a mod P, as
 * lanczos_modp --signed solves it.
 * --wide (no reference counterpart) reads the matrix in wide value mode: an entry is any int64 and means its residue mod P,
 * as lanczos_modp --wide solves it.
 */
#define _GNU_SOURCE
#include <err.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>

#include "blz.h"

int main(int argc, char **argv)
{
	struct option longopts[] = {
		{"matrix", required_argument, NULL, 'm'}, {"kernel", required_argument, NULL, 'k'},
		{"prime", required_argument, NULL, 'p'}, {"right", no_argument, NULL, 'r'},
		{"left", no_argument, NULL, 'l'}, {"independent", no_argument, NULL, 'i'},
		{"rhs", required_argument, NULL, 'b'}, {"signed", no_argument, NULL, 's'}, {"wide", no_argument, NULL, 'w'},
		{NULL, 0, NULL, 0}
	};
	char *matrix = NULL, *kernel = NULL, *rhs = NULL;
	unsigned long long prime = 0;
	int right = 0, independent = 0, sgn = 0, wide = 0, ch;
	while ((ch = getopt_long(argc, argv, "", longopts, NULL)) != -1) {
		switch (ch) {
		case 'm': matrix = optarg; break;
		case 'k': kernel = optarg; break;
		case 'p': prime = strtoull(optarg, NULL, 10); break;
		case 'r': right = 1; break;
		case 'l': right = 0; break;
		case 'i': independent = 1; break;
		case 'b': rhs = optarg; break;
		case 's': sgn = 1; break;
		case 'w': wide = 1; break;
		default: errx(1, "Unknown option\n");
		}
	}
	if (matrix == NULL || kernel == NULL || prime == 0 || (wide && sgn)) {
		printf("%s [OPTIONS]\n\n", argv[0]);
		printf("Options:\n");
		printf("--matrix FILENAME           MatrixMarket file containing the sparse matrix\n");
		printf("--kernel FILENAME           MatrixMarket file containing the kernel vectors\n");
		printf("--prime P                   compute modulo P (up to 2**62)\n");
		printf("--right                     check right kernel vectors\n");
		printf("--left                      check left kernel vectors [default]\n");
		printf("--independent               also check that the kernel vectors are linearly independent\n");
		printf("--rhs FILENAME              check a solution: --kernel holds x, FILENAME holds b, and M*x == b (--right)\n");
		printf("                            or x*M == b (--left) is verified\n");
		printf("--signed                    signed value mode: a matrix entry a (an int32) means a mod P, so -1 is P-1\n");
		printf("                            (what lanczos_modp --signed solves; P < 2**62)\n");
		printf("--wide                      wide value mode: a matrix entry is any int64 and means its residue mod P\n");
		printf("                            (what lanczos_modp --wide solves; P < 2**62; not with --signed)\n");
		exit(0);
	}
	if (rhs) {
		printf("Reading Matrix from %s, solution from %s and right-hand side from %s\n", matrix, kernel, rhs);
		int k = 0;
		blz_rhs_load_block(rhs, prime, -1, BLZ_MAX_RHS, &k, NULL);	/* the size line only; one column: as ever, below */
		if (k > 1) {
			int status[BLZ_MAX_RHS], failed = 0;
			int64_t bad_row[BLZ_MAX_RHS];
			const int kk = wide ? blz_check_solution_block_wide(matrix, rhs, kernel, prime, right, status, bad_row)
				     : sgn ? blz_check_solution_block_signed(matrix, rhs, kernel, prime, right, status, bad_row)
					   : blz_check_solution_block(matrix, rhs, kernel, prime, right, status, bad_row);
			if (kk < 0)
				errx(1, "%s", blz_last_error());
			for (int i = 0; i < kk; i++) {
				if (status[i] == 0)
					printf("OK\n");
				else if (status[i] == 3)
					printf("KO: no solution (rhs %d, x is zero)\n", i);
				else
					printf("KO: %s != b (rhs %d, row %lld)\n", right ? "M*x" : "x*M", i, (long long)bad_row[i]);
				failed += status[i] == 2;
			}
			exit(failed ? EXIT_FAILURE : EXIT_SUCCESS);
		}
		int64_t bad = 0;
		const int rcs = wide ? blz_check_solution_wide(matrix, rhs, kernel, prime, right, &bad)
				: sgn ? blz_check_solution_signed(matrix, rhs, kernel, prime, right, &bad)
				    : blz_check_solution(matrix, rhs, kernel, prime, right, &bad);
		if (rcs == 0) {
			printf("OK\n");
			exit(EXIT_SUCCESS);
		}
		if (rcs == 2) {
			printf("KO: %s != b (row %lld)\n", right ? "M*x" : "x*M", (long long)bad);
			exit(EXIT_FAILURE);
		}
		errx(1, "%s", blz_last_error());
	}
	printf("Reading Matrix from %s and kernel from %s\n", matrix, kernel);
	long long row = 0;
	int col = 0;
	const int rc = wide ? blz_check_kernel_wide(matrix, kernel, prime, right, (int64_t *)&row, &col)
		     : sgn ? blz_check_kernel_signed(matrix, kernel, prime, right, (int64_t *)&row, &col)
			   : blz_check_kernel(matrix, kernel, prime, right, (int64_t *)&row, &col);
	if (rc == 0) {
		printf("OK\n");
		if (independent) {
			int rank = 0, cols = 0;
			if (blz_check_independent(kernel, prime, &rank, &cols) != BLZ_OK)
				errx(1, "%s", blz_last_error());
			if (rank < cols)
				errx(1, "KO: kernel vectors are linearly dependent (rank %d < %d)", rank, cols);
			printf("OK: %d independent vectors\n", cols);
		}
		exit(EXIT_SUCCESS);
	}
	if (rc == 1)
		errx(1, "KO: kernel vectors are all zero");
	if (rc == 2)
		errx(1, "KO: y[%lld, %d] != 0\n", row, col);
	errx(1, "%s", blz_last_error());
}
