"""Beyond the reference's domain (p > 2^32: it stores u32 and caps p at 2^30-35,
sequential/lanczos_modp.c:189-193) no reference output can exist.  Here the
oracle's SAME code path (already pinned to the reference at small p by
test_oracle_golden.py) is cross-checked at p = 2^61-1 and other wide primes against
an independent restatement in exact Python integers (tests/exact_ref.py), and against the reference's
own in-loop invariants (correctness_tests / final_check,
sequential/lanczos_modp.c:532-582).
"""
import os

import numpy as np
import pytest

import oracle as orc
from exact_ref import iteration as py_iteration

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P61 = (1 << 61) - 1
WIDE_PRIMES = [P61, (1 << 31) - 1, 4294967311, 2305843009213693907, (1 << 62) - 57]


@pytest.mark.parametrize("p", WIDE_PRIMES)
@pytest.mark.parametrize("name,n,right", [("quirks40x30", 2, False), ("quirks40x30", 3, True),
                                          ("trefethen20", 4, False)])
def test_wide_prime_trajectory_vs_python_ints(p, name, n, right):
    M = orc.Matrix.load(os.path.join(GOLDEN, name + ".mtx"), p)
    nrows = M.ncols if right else M.nrows
    recs = []
    res = orc.block_lanczos(M, n, p, right=right, trace=recs.append)
    v = [int(x) for x in orc.init_v(nrows, n, p)]
    pb = [0] * (nrows * n)
    for k, r in enumerate(recs):
        assert [int(x) for x in r["v"]] == v
        npiv, v, pb, tmp, (vtAv, vtAAv, winv, d) = py_iteration(M, n, p, right, v, pb)
        assert r["npiv"] == npiv
        assert [int(x) for x in r["vtAv"]] == vtAv and [int(x) for x in r["vtAAv"]] == vtAAv
        assert [int(x) for x in r["winv"]] == winv and [int(x) for x in r["d"]] == d
        assert [int(x) for x in r["tmp"]] == tmp
    assert recs[-1]["npiv"] == 0
    assert [int(x) for x in res["v"]] == v


@pytest.mark.parametrize("p", [P61, 1073741789])
def test_invariants_of_reference_correctness_tests(p):
    """sequential/lanczos_modp.c:532-557 evaluated on the oracle at 64 bits, and final_check :560-582."""
    n = 4
    M = orc.Matrix.load(os.path.join(GOLDEN, "rand300x200.mtx"), p)
    recs = []
    res = orc.block_lanczos(M, n, p, trace=recs.append)
    for r in recs:
        A, B, W, d = (r[k].astype(object) for k in ("vtAv", "vtAAv", "winv", "d"))
        A, B, W = A.reshape(n, n), B.reshape(n, n), W.reshape(n, n)
        assert (A == A.T).all() and (B == B.T).all() and (W == W.T).all()
        for i in range(n):
            for j in range(n):
                assert W[i, j] == 0 or d[i] or d[j]
        D = np.diag(d)
        assert ((W.dot(A.dot(D))) % p == D).all()
    assert orc.final_check(M.nrows, M.ncols, n, res["v"], res["tmp"]) == 3  # v != 0 and v^T M == 0
    y = orc.spmv(M, res["v"], True, n, p)
    assert not y.any()


def test_omp_kernels_equal_sequential_at_wide_prime():
    p, n = P61, 8
    M = orc.Matrix.load(os.path.join(GOLDEN, "rand3000x2000.mtx"), p)
    v = orc.init_v(M.nrows, n, p)
    t = orc.spmv(M, v, True, n, p)
    assert np.array_equal(orc.spmv_omp(M, v, True, n, p, 4), t)
    Av = orc.spmv(M, t, False, n, p)
    assert np.array_equal(orc.spmv_omp(M, t, False, n, p, 4), Av)
    a, b = orc.block_dot(M.nrows, Av, v, n, p)
    a2, b2 = orc.block_dot(M.nrows, Av, v, n, p, omp_threads=4)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    # one whole OpenMP iteration == one oracle iteration
    res = orc.block_lanczos(M, n, p, stop_after=1)
    vv, tt, aa, pp = v.copy(), np.zeros(max(M.nrows, M.ncols) * n, np.uint64), np.zeros(M.nrows * n, np.uint64), \
        np.zeros(M.nrows * n, np.uint64)
    assert orc.iteration_omp(M, n, p, False, vv, tt, aa, pp, 4) > 0
    assert np.array_equal(vv, res["v"]) and np.array_equal(pp, res["p"])


@pytest.mark.parametrize("p,n,right", [(P61, 8, False), (1073741789, 4, True), ((1 << 62) - 57, 3, False)])
def test_by_rows_omp_iteration_equals_sequential(p, n, right):
    """orc_iteration_csr_omp (CSR built once, one output row per loop iteration, no per-thread copies of the output):
    the form bench.py times as cpu_baseline.  Same words as the sequential restatement, for both products and over
    several whole iterations."""
    M = orc.Matrix.load(os.path.join(GOLDEN, "rand3000x2000.mtx"), p)
    pair = orc.CsrPair(M)
    rows_v = M.ncols if right else M.nrows
    x = orc.init_v(M.ncols, n, p)
    assert np.array_equal(pair.spmv(x, False, n, p, 4), orc.spmv(M, x, False, n, p))
    y = orc.init_v(M.nrows, n, p)
    assert np.array_equal(pair.spmv(y, True, n, p, 3), orc.spmv(M, y, True, n, p))
    want = orc.block_lanczos(M, n, p, right=right, stop_after=4)
    v = orc.init_v(rows_v, n, p)
    tmp, Av, pb = np.zeros(max(M.nrows, M.ncols) * n, np.uint64), np.zeros(rows_v * n, np.uint64), np.zeros(rows_v * n, np.uint64)
    for _ in range(4):
        assert pair.iteration(n, p, right, v, tmp, Av, pb, 4) > 0
    pair.close()
    assert np.array_equal(v, want["v"]) and np.array_equal(pb, want["p"])
