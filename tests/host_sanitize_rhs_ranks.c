/* blz_gathered_position and blz_rhs_cut (the host arithmetic of the bordered solve on several ranks) under
 * AddressSanitizer + UBSan (CPU build), error paths included.  Compiled and run by tests/test_host_rhs_ranks.py. */
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

int main(void)
{
	/* every row of a partition with an empty rank and a rank that fills its slab, at every piece count that divides the stride:
	 * the positions are distinct, below nranks * stride, and piece k of every rank is contiguous */
	const int64_t bounds[] = { 0, 12, 12, 17, 40, 41 };
	const int nranks = 5;
	for (int chunks = 1; chunks <= 6; chunks++) {
		const int64_t stride = 24;	/* >= the largest slab (23 rows), a multiple of 1, 2, 3, 4, 6 */
		if (stride % chunks) {
			REQUIRE(blz_gathered_position(bounds, nranks, stride, chunks, 0, NULL, NULL) == BLZ_EINVAL);
			continue;
		}
		const int64_t piece = stride / chunks;
		char *seen = calloc((size_t)(nranks * stride), 1);
		REQUIRE(seen != NULL);
		for (int64_t row = 0; row < 41; row++) {
			int owner = -1;
			int64_t local = -1;
			const int64_t pos = blz_gathered_position(bounds, nranks, stride, chunks, row, &owner, &local);
			REQUIRE(pos >= 0 && pos < nranks * stride && !seen[pos]);
			seen[pos] = 1;
			REQUIRE(owner >= 0 && owner < nranks && bounds[owner] <= row && row < bounds[owner + 1] && local == row - bounds[owner]);
			REQUIRE(pos == (local / piece) * (nranks * piece) + owner * piece + local % piece);
			REQUIRE(blz_gathered_position(bounds, nranks, stride, chunks, row, NULL, NULL) == pos);
		}
		free(seen);
		REQUIRE(blz_gathered_position(bounds, nranks, stride, chunks, 41, NULL, NULL) == BLZ_EINVAL);
		REQUIRE(blz_gathered_position(bounds, nranks, stride, chunks, -1, NULL, NULL) == BLZ_EINVAL);
	}
	REQUIRE(blz_gathered_position(bounds, nranks, 20, 1, 39, NULL, NULL) == BLZ_EINVAL);	/* row 22 of rank 3, a slab has 20 */
	REQUIRE(blz_gathered_position(NULL, nranks, 24, 1, 0, NULL, NULL) == BLZ_EINVAL);
	REQUIRE(blz_gathered_position(bounds, 0, 24, 1, 0, NULL, NULL) == BLZ_EINVAL);
	const int64_t one[] = { 0, 9 };		/* one rank: the identity */
	for (int64_t row = 0; row < 9; row++)
		REQUIRE(blz_gathered_position(one, 1, 9, 3, row, NULL, NULL) == row);

	/* the cut: exactly count * kp words written (max(count, 1) * kp for an empty rank), padding zero, rows placed by perm */
	const uint64_t p = (1ull << 61) - 1;
	enum { LEN = 7, K = 3, KP = 4 };
	uint64_t b[LEN * K];
	for (int q = 0; q < LEN * K; q++)
		b[q] = (uint64_t)(q + 1) * 1000003u % p;
	const int32_t perm[LEN] = { 6, 0, 5, 1, 4, 2, 3 };
	for (int64_t first = 0; first <= LEN; first++)
		for (int64_t count = 0; first + count <= LEN; count++)
			for (int with_perm = 0; with_perm < 2; with_perm++) {
				const size_t words = (size_t)(count > 0 ? count : 1) * KP;
				uint64_t *out = malloc((words + 1) * sizeof *out);	/* exact size: one word more is ASan's business */
				REQUIRE(out != NULL);
				memset(out, 0xAB, (words + 1) * sizeof *out);
				REQUIRE(blz_rhs_cut(b, LEN, K, KP, p, with_perm ? perm : NULL, first, count, out) == BLZ_OK);
				REQUIRE(out[words] == 0xABABABABABABABABull);
				for (int64_t r = 0; r < LEN; r++) {
					const int64_t at = with_perm ? perm[r] : r;
					if (at < first || at >= first + count)
						continue;
					for (int i = 0; i < KP; i++)
						REQUIRE(out[(at - first) * KP + i] == (i < K ? b[r * K + i] : 0));
				}
				if (count == 0)
					for (int i = 0; i < KP; i++)
						REQUIRE(out[i] == 0);
				free(out);
			}
	{	/* k == 1 keeps one word per row; a word that is not a residue is refused whoever owns its row */
		uint64_t out[LEN], one_col[LEN] = { 1, 2, 3, 4, 5, 6, 7 };
		REQUIRE(blz_rhs_cut(one_col, LEN, 1, 1, p, NULL, 2, 3, out) == BLZ_OK && out[0] == 3 && out[2] == 5);
		one_col[6] = p;
		REQUIRE(blz_rhs_cut(one_col, LEN, 1, 1, p, NULL, 2, 3, out) == BLZ_EINVAL && strstr(blz_last_error(), "not below p"));
		REQUIRE(blz_rhs_cut(one_col, LEN, 1, 1, p, NULL, 5, 3, out) == BLZ_EINVAL);	/* rows past the end */
		REQUIRE(blz_rhs_cut(one_col, LEN, 2, 1, p, NULL, 0, 1, out) == BLZ_EINVAL);	/* kp < k */
		REQUIRE(blz_rhs_cut(NULL, LEN, 1, 1, p, NULL, 0, 1, out) == BLZ_EINVAL);
	}
	printf("rhs ranks host code clean under ASan + UBSan\n");
	return 0;
}
