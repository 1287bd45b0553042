"""rhs_ref (tests/rhs_ref.py) held to itself and to the CPU oracle: the bordered operator written out as a matrix.

CPU only.  What the GPU tests of the right-hand-side solve lean on is pinned here: the augmented triplets, the planted
systems and which of them have a unique solution, the Gaussian elimination, and -- at primes below 2^32, where the
border fits the oracle's 32-bit values -- exact_ref's trajectory on the augmented matrix against the oracle's
block_lanczos word for word."""
import os

import numpy as np
import pytest

import exact_ref as X
import oracle as orc
import rhs_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P61 = X.P61


def mtx(name, p):
    return X.load_mtx(os.path.join(GOLDEN, name + ".mtx"), p)


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (65537, (1 << 31) - 1, P61, X.largest_prime_below(1 << 62)))
def test_planted_solution_is_a_kernel_vector_of_the_augmented_matrix(p, right):
    M = mtx("quirks40x30", p)
    x0, b = R.planted(M, right, p, 1)
    A = R.augmented(M, b, right)
    assert (A.nrows, A.ncols) == ((M.nrows, M.ncols + 1) if right else (M.nrows + 1, M.ncols))
    assert max(int(w) for w in A.x) < p and A.nnz == M.nnz + sum(1 for w in b if w)
    v = x0 + [p - 1]                                    # (x0, -1): M x0 - b = 0
    assert not any(X.spmv(A, v, not right, 1, p))
    assert R.from_kernel([w * 12345 % p for w in v], p) == x0
    assert not any(R.residual(M, x0, b, right, p))
    # an unknown the matrix really uses (quirks40x30 has empty and cancelling lines): moving it breaks the system
    k = next(k for k in range(len(x0)) if any(R.apply(M, [int(q == k) for q in range(len(x0))], right, p)))
    bad = list(x0)
    bad[k] = (bad[k] + 1) % p
    assert any(R.residual(M, bad, b, right, p))


@pytest.mark.parametrize("name,right,unique", (("rand300x200", True, True), ("wide120x260", False, True),
                                               ("rand300x200", False, False), ("wide120x260", True, False),
                                               ("quirks40x30", True, False), ("quirks40x30", False, False)))
def test_which_planted_systems_have_one_solution(name, right, unique):
    for p in (65537, (1 << 31) - 1, P61):
        M = mtx(name, p)
        x0, b = R.planted(M, right, p, 2)
        rank, x, uniq = R.solve(M, b, right, p)
        assert x is not None and not any(R.residual(M, x, b, right, p))
        assert uniq == unique, (name, right, p, rank)
        if unique:
            assert x == x0


def test_a_random_rhs_on_the_tall_matrix_has_no_solution():
    for p in (65537, (1 << 31) - 1, P61):
        M = mtx("rand300x200", p)
        rank, x, _ = R.solve(M, R.random_rhs(M, True, p, 3), True, p)
        assert rank == 200 and x is None


@pytest.mark.parametrize("name,right,n,p", (("quirks40x30", True, 4, 65537), ("quirks40x30", False, 2, (1 << 31) - 1),
                                            ("wide120x260", False, 8, 1073741789), ("rand300x200", True, 8, 65537)))
def test_exact_trajectory_on_the_augmented_matrix_is_the_oracles(name, right, n, p):
    M = mtx(name, p)
    x0, b = R.planted(M, right, p, 4)
    A = R.augmented(M, b, right)
    recs, end = X.trajectory(A, n, p, right)
    assert recs[0]["v"] == R.init_v(M, right, n, p)
    want = orc.block_lanczos(orc.Matrix(A.nrows, A.ncols, A.i, A.j, A.x), n, p, right=right)
    assert end["iterations"] == want["iterations"]
    assert np.array_equal(R.as_u64(end["v"]), want["v"]) and np.array_equal(R.as_u64(end["p"]), want["p"])
    # every column of the final block is a kernel vector of the augmented matrix; one with a non-zero last word solves
    V = np.array(end["v"], dtype=object).reshape(-1, n)
    assert not any(end["tmp"])
    cols = [j for j in range(n) if V[-1, j]]
    assert cols
    x = R.from_kernel(list(V[:, cols[0]]), p)
    assert not any(R.residual(M, x, b, right, p))
    if (name, right) in (("rand300x200", True), ("wide120x260", False)):
        assert x == x0
