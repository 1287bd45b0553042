"""fused_ref (the closed form tests/test_gpu_fused_dot.py compares the fused inner products with) held against exact_ref
and the C oracle, and the condition that makes the GPU tests able to fail: one product too many of the words the closed
form's inputs hold overflows the reducer, at every prime whose reducer has no more room than make_modp's chunk uses.
No GPU needed."""
import numpy as np
import pytest

import exact_ref as X
import fused_ref as F
import oracle as orc

LADDER = X.ladder()
WIDTHS = (1, 2, 3, 4, 8)


def small_cases():
    """Every builder and value mode at a size Python integers handle: a hot column, long rows, empty rows, duplicates."""
    lad = F.ladder((0, 1, 3, 4, 5, 17, 40), repeat=2, mode="array", seed=3)
    return {
        "perm_id": F.perm(23, None, "ones"),
        "perm_rand": F.perm(23, 5, "palette"),
        "ladder": lad,
        "hot": F.hot(31, 29, 3, 4, "palette", seed=2),
        "hot_dups": F.hot(12, 6, 5, 2, "ones", seed=1),          # 5 draws from 4 columns: repeated (row, column) pairs
        "band": F.band(19, 4, "ones"),
        "mixed": F.shuffled_rows(F.mixed([F.perm(7, 1), lad, F.hot(9, 8, 2, 3, "array", seed=4)]), seed=6),
    }


SMALL = small_cases()


def test_builders_give_what_they_promise():
    for R, seed in ((50, None), (50, 3)):
        A = F.perm(R, seed)
        assert sorted(A.i) == list(range(R)) and sorted(A.j) == list(range(R))
    A = F.ladder((0, 1, 5, 4097), repeat=3)
    assert np.bincount(A.i, minlength=A.nrows).tolist() == [0, 1, 5, 4097] * 3 + [0, 0]
    assert np.bincount(A.j, minlength=A.ncols).max() == 1
    A = F.hot(1000, 900, 6, 16)
    cols = np.bincount(A.j, minlength=A.ncols)
    assert cols[:16].sum() * 4 == A.nnz and (np.bincount(A.i) == 8).all()
    A = SMALL["hot_dups"]
    assert len(set(zip(A.i.tolist(), A.j.tolist()))) < A.nnz, "this case is meant to hold duplicates"
    assert len(np.unique(F.values(5000, "palette"))) <= 256 < len(np.unique(F.values(5000, "array")))
    assert (F.values(7, "ones") == 1).all()
    for A in SMALL.values():
        assert A.x.min() >= 1 and A.x.max() <= 1000 and A.i.max() < A.nrows and A.j.max() < A.ncols
    B = F.mixed([F.perm(3), F.perm(4)])
    assert (B.nrows, B.ncols, B.nnz) == (7, 7, 7) and B.j.tolist() == [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_closed_form_against_exact_integers(name, right):
    A = SMALL[name]
    nr, nc, i, j, x = F.as_matrix(A, right)
    for p in LADDER:
        M = X.Coo(nr, nc, i, j, x % p)
        for n in WIDTHS:
            for kind in ("ramp", "max"):
                e = F.expect(A, n, p, kind)
                v = [int(w) for w in e["v"]]
                assert len(v) == (nc if right else nr) * n
                tmp = X.spmv(M, v, not right, n, p)
                Av = X.spmv(M, tmp, right, n, p)
                a, b = X.block_dot(A.nrows, Av, v, n, p)
                assert tmp == [int(w) for w in e["tmp"]], (p, n, kind)
                assert Av == [int(w) for w in e["Av"]], (p, n, kind)
                assert a == [int(w) for w in e["vtAv"]] and b == [int(w) for w in e["vtAAv"]], (p, n, kind)


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
def test_closed_form_against_the_oracle_at_1e5_rows(right):
    lengths = (0, 1, 3, 4, 5, 63, 64, 65, 300, 4097)
    A = F.shuffled_rows(F.mixed([F.perm(60000, 7, "array"), F.ladder(lengths, repeat=30, mode="palette", seed=1),
                                 F.hot(40000, 30000, 5, 37, "ones", seed=9)]), seed=11)
    assert A.nrows > 10 ** 5
    nr, nc, i, j, x = F.as_matrix(A, right)
    for p, n in ((X.largest_prime_below(1 << 57), 8), (X.P61, 4), ((1 << 62) - 57, 8), (X.P31, 5), (65537, 2)):
        M = orc.Matrix(nr, nc, i, j, x % p)
        for kind in ("ramp", "max"):
            e = F.expect(A, n, p, kind)
            tmp = orc.spmv_omp(M, e["v"], not right, n, p)
            Av = orc.spmv_omp(M, tmp, right, n, p)
            a, b = orc.block_dot(A.nrows, Av, e["v"], n, p, omp_threads=8)
            assert np.array_equal(tmp, e["tmp"]) and np.array_equal(Av, e["Av"]), (p, n, kind)
            assert np.array_equal(a, e["vtAv"]) and np.array_equal(b, e["vtAAv"]), (p, n, kind)


def reducer_bound(p):
    return 1 << 128 if p == X.P61 else 1 << (63 + p.bit_length())


TIGHT = [p for p in LADDER if X.chunk(p) < 64 or p.bit_length() == 57]
# the 57- to 62-bit primes of tests/test_gpu_fused_dot.py: the largest of every bit length, both 61-bit reducers
GPU_PRIMES = [X.largest_prime_below(1 << k) for k in (57, 58, 59, 60, 62)] + [X.P61, X.largest_prime_below(X.P61)]


def test_one_product_too_many_of_these_words_overflows_the_reducer():
    """The inputs alone: at every prime whose chunk is below 64, or of 57 bits, slack(p) + 1 products of the smallest
    non-zero words the closed form's v and Av can hold (p - n and p - 2^40, n <= 8) exceed the reducer's bound, while
    slack(p) products of the largest (p - 1) plus a residue fit -- so for these words "products that fit" is slack(p)
    exactly as for (p-1)^2, and a sum that takes more than slack(p) of them gives a wrong word."""
    assert {p.bit_length() for p in TIGHT} == {57, 58, 59, 60, 61, 62}
    assert X.P61 in TIGHT and X.largest_prime_below(1 << 57) in TIGHT
    tight = 0
    for p in TIGHT:
        lo_v, lo_av = F.smallest_words(8, p)
        fit = X.slack(p)
        assert fit * (p - 1) ** 2 + (p - 1) < reducer_bound(p)
        if p - (1 << (p.bit_length() - 1)) < 1 << 20:
            # The smallest primes of a bit length (2^(k-1) + a few): the reducer's bound is 2^(63+k) whatever p is, so it
            # leaves room for about four times chunk products there, and slack(p) + 1 products pass it only if every word
            # is within p - 2^(k-1) < 100 of p, which no block of a product is.  No miscount by one or two products can
            # show at these primes; the GPU tests do not use them.
            assert fit > 3 * X.chunk(p) and p not in GPU_PRIMES
            continue
        tight += 1
        for a, b in ((lo_v, lo_av), (lo_av, lo_av)):                   # a product of v^T Av, of Av^T Av
            assert (fit + 1) * a * b >= reducer_bound(p), (p, fit)
    assert tight == 7 and all(p in TIGHT for p in GPU_PRIMES)
    # at the largest Barrett prime of every class chunk + 2 products (the rows per accumulator the GPU tests give) are
    # more than fit: chunk + 1 at 57 bits, where nothing is left over
    for k in (57, 58, 59, 60, 61, 62):
        p = X.largest_prime_below(X.P61 if k == 61 else 1 << k)
        assert X.slack(p) == X.chunk(p) + (0 if k == 57 else 1), k
    assert X.slack(X.P61) == 64 and X.chunk(X.P61) == 32        # folding: two skipped reductions overflow, not one


def test_the_totals_are_not_zero_at_the_test_primes():
    """sum s_c and sum s_c^2 are far below the 56- to 62-bit primes (so never 0 mod p) for matrices of the sizes used."""
    A = SMALL["mixed"]
    e = F.expect(A, 8, X.P61, "ramp")
    assert 0 < e["sum_s"] < 1 << 50 and 0 < e["sum_s2"] < 1 << 56
    assert e["sum_s"] == int(sum(int(c) ** 2 for c in F.column_and_row_sums(A, X.P61, 8)[0]))
