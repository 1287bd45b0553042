"""The kernels against exact integers at every reducer class of csrc/modp.h.

make_modp() sets `chunk`, how many products of two residues a dense sum may take before a reduction, from k, the bit
length of p; ortho_dispatch / dot_dispatch pick their kernels from chunk and n.  At the largest prime below each 2^k
(third column: products of (p-1)^2, plus one residue, that still fit the reducer -- 2^(63+k) Barrett, 2^128 folding):

    k (bits of p)        chunk  fit   update kernel by width
    <= 56                64     >=128 fast n <= 16, _32, _64
    57                   64     64    fast n <= 16, _32, _64     (no slack: one product too many is a wrong word)
    58                   31     32    fast n <= 8; generic n >= 16
    59                   15     16    fast n <= 4; generic n >= 8
    60                   7      8     fast n <= 2; generic n >= 4
    61, Barrett          3      4     fast n = 1; generic n >= 2
    61, 2^61-1 folding   32     64    fast n <= 16, _32, _64
    62                   1      2     generic for every n

A. the exact_*.npz trajectories (tests/golden/make_exact_golden.py, exact integers only), iteration by iteration,
   under the default plan, BLZ_NO_MFMA=1, BLZ_MFMA_MIN_ROWS=0 and BLZ_NO_FUSE=1;
B. semi_inverse / orthogonalize / block_dot step by step at the ladder primes and widths 1 ... 64 (and exact widths
   under BLZ_NO_PAD=1), against exact_ref (the oracle where Python integers would be too slow; test_exact_ref.py pins
   it to exact_ref at every ladder prime), and all-(p-1) blocks long enough that every inner-product accumulator
   takes more than chunk products;
C. SpMV with every value 2^32-1 mod p (p-1 where p divides 2^32-1) and every operand p-1, rows of 1 ... 20000
   entries, both orientations, the staged form forced on and off: closed-form expectations;
D. block_rref and kernel_basis (k_rref, k_block_mul) at the 57-62-bit Barrett primes, at widths the kernel-basis
   tests skip, padded and exact, against kbasis_ref; and the edge nranks * p <= 2^64 of the all-reduce on loopback
   ranks.

block_dot() above is the stand-alone kernel; the same products as the epilogue of the second SpMV (widths 1 ... 8, six
kernels) are held to exact integers by tests/test_gpu_fused_dot.py.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import blz
import exact_ref as X
import kbasis_ref as kb
import oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT = sorted(glob.glob(os.path.join(GOLDEN, "exact_*.npz")))
P61 = X.P61
P57 = X.largest_prime_below(1 << 57)
LADDER = X.ladder()
# every width and every cell at the tight 57-bit prime and at 2^61-1; the other primes are sampled
FULL = (P57, P61)
EDGE = tuple(X.largest_prime_below(1 << k) for k in (58, 59, 60)) + (X.largest_prime_below(P61),
                                                                    X.largest_prime_below(1 << 62))
OTHER = (3, 65537, (1 << 31) - 1, 4294967291, 4294967311, X.largest_prime_below(1 << 48),
         X.largest_prime_below(1 << 56))
WIDTHS = (1, 2, 3, 4, 8, 16, 24, 32, 64)
EXACT_WIDTHS = (3, 24, 33, 48, 63)        # under BLZ_NO_PAD=1: the generic kernels at their own width
PY_PRODUCTS = 2 * 10 ** 5                 # above this, the oracle stands in for exact_ref (and for semi_inverse at n > 24)


def device_cus():
    """Compute units of device 0 as the HIP runtime reports them (hipDeviceGetAttribute, the count the library sizes
    its grids by).  The attribute numbers are those of hip_runtime_api.h; MaxThreadsPerBlock = 1024 checks them."""
    hip = C.CDLL("libamdhip64.so")
    mp, threads = C.c_int(0), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(threads), 56, 0) == 0 and threads.value == 1024
    assert hip.hipDeviceGetAttribute(C.byref(mp), 63, 0) == 0 and mp.value > 0
    return mp.value


def pow2(n):
    w = 1
    while w < n:
        w <<= 1
    return w


def ints(a):
    return [int(w) for w in np.asarray(a).reshape(-1)]


def update_kernel(p, n, padded=True):
    """The update kernel ortho_dispatch picks on the vector ALU (BLZ_NO_MFMA=1 / below BLZ_MFMA_MIN_ROWS)."""
    w = n
    if padded:
        while w & (w - 1):
            w += 1
    c = X.chunk(p)
    if w == 64 and c >= 32:
        return "_64"
    if w == 32 and c >= 32:
        return "_32"
    if w in (1, 2, 4, 8, 16) and c >= 2 * w:
        return "fast"
    return "generic"


def step_cases():
    out = [(p, n, True) for p in FULL for n in WIDTHS] + [(p, n, False) for p in FULL for n in EXACT_WIDTHS]
    out += [(p, n, True) for p in EDGE for n in (1, 2, 4, 8, 16, 64)] + [(p, 24, False) for p in EDGE]
    out += [(p, n, True) for p in OTHER for n in (2, 8, 32, 64)]
    return out


STEP_CASES = step_cases()


def test_the_cases_reach_every_cell_of_the_table():
    """Every (chunk class, update kernel) pair the table lists is exercised by STEP_CASES, and the table is what
    exact_ref.chunk (make_modp) gives."""
    want = {57: {"fast", "_32", "_64"}, 58: {"fast", "generic"}, 59: {"fast", "generic"}, 60: {"fast", "generic"},
            "61b": {"fast", "generic"}, "61f": {"fast", "_32", "_64"}, 62: {"generic"}}
    fast_max = {57: 16, 58: 8, 59: 4, 60: 2, "61b": 1, "61f": 16}
    got = {}
    for p, n, padded in STEP_CASES:
        k = p.bit_length()
        key = ("61f" if p == P61 else "61b") if k == 61 else k
        got.setdefault(key, set()).add(update_kernel(p, n, padded))
        if key in fast_max and padded and n in (1, 2, 4, 8, 16):
            assert (update_kernel(p, n) == "fast") == (n <= fast_max[key]), (key, n)
    for key, kernels in want.items():
        assert kernels <= got[key], (key, got.get(key))
    assert {X.chunk(p) for p in FULL + EDGE} == {64, 31, 15, 7, 3, 32, 1}
    assert all(p in LADDER for p in FULL + EDGE + OTHER)


# ------------------------------------------------------------------------------------------------ A. fixtures


def fixture_matrix(g, p):
    name = str(g["matrix"])
    if name == "synth":
        nr, nc, nz, seed = (int(x) for x in g["synth"])
        M = blz.Matrix.synth(nr, nc, nz, seed, p)
    else:
        M = blz.Matrix.load(os.path.join(GOLDEN, name + ".mtx"), p)
    assert X.coo_sha(M.i, M.j, M.x) == str(g["coo_sha"]), "the matrix generator changed"
    return M


@pytest.mark.parametrize("env", ["default", "BLZ_NO_MFMA", "BLZ_MFMA_MIN_ROWS", "BLZ_NO_FUSE"])
@pytest.mark.parametrize("path", EXACT, ids=[os.path.basename(p)[6:-4] for p in EXACT])
def test_exact_trajectory(monkeypatch, path, env):
    if env != "default":
        monkeypatch.setenv(env, "0" if env == "BLZ_MFMA_MIN_ROWS" else "1")
    g = np.load(path)
    p, n, right, stop = int(g["prime"]), int(g["n"]), bool(g["right"]), int(g["stop_after"])
    M = fixture_matrix(g, p)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M, right)
        ctx.init_v()
        for k in range(len(g["npiv"])):
            if stop > 0 and k == stop:
                break
            assert X.sha(ctx.get_block(blz.V)) == str(g["vhash"][k]), k
            done, stopped, _ = ctx.iterate(1)
            for which, name in ((blz.VTAV, "vtAv"), (blz.VTAAV, "vtAAv"), (blz.WINV, "winv"), (blz.D, "d")):
                assert np.array_equal(ctx.get_small(which), g[name][k]), (name, k)
            assert stopped == (g["npiv"][k] == 0) and done == (0 if stopped else 1)
        assert ctx.iterations == int(g["iterations"])
        for blk, key in ((blz.V, "v"), (blz.P, "p"), (blz.TMP, "tmp")):
            if key == "tmp" and stop > 0:
                continue
            got = ctx.get_block(blk)
            if "final_" + key in g.files:
                assert np.array_equal(got, g["final_" + key]), key
            else:
                assert X.sha(got) == str(g["final_" + key + "_sha"]), key


# ------------------------------------------------------------------------------------------------ B. step by step


def tall(rows):
    """A matrix with `rows` rows and a few entries: the blocks V, AV, P get `rows` rows."""
    return blz.Matrix(rows, 3, [0, rows - 1], [0, 2], [1, 1])


def expect_update(v, Av, pb, d, S, B, winv, rows, n, p):
    if rows * n * n * 3 <= PY_PRODUCTS:
        return X.orthogonalize(v, pb, d, S, B, winv, rows, Av, n, p)
    got = orc.orthogonalize(np.array(v, np.uint64), np.array(pb, np.uint64), d, S, B, winv, rows,
                            np.array(Av, np.uint64), n, p)
    return [int(w) for w in got[0]], [int(w) for w in got[1]]


def expect_semi(A, n, p):
    if n <= 24:
        return X.semi_inverse(A, n, p)
    npiv, winv, d = orc.semi_inverse(np.array(A, np.uint64), n, p)
    return npiv, [int(w) for w in winv], [int(w) for w in d]


def expect_dot(v, Av, rows, n, p):
    if rows * n * n * 2 <= PY_PRODUCTS:
        return X.block_dot(rows, Av, v, n, p)
    a, b = orc.block_dot(rows, np.array(Av, np.uint64), np.array(v, np.uint64), n, p, omp_threads=8)
    return [int(w) for w in a], [int(w) for w in b]


@pytest.mark.parametrize("p,n,padded", STEP_CASES,
                         ids=[f"p{p.bit_length()}b{'f' if p == P61 else ''}-n{n}{'' if pd else '-nopad'}-{p % 1000}"
                              for p, n, pd in STEP_CASES])
def test_steps_against_exact_integers(monkeypatch, p, n, padded):
    monkeypatch.setenv("BLZ_NO_PAD", "0" if padded else "1")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    full = p in FULL
    rows_list = (1, 2, 255, 256, 257, 4099) if full else (1, 257, 4099)
    with blz.Context(p, n) as ctx:
        # semi_inverse alone, on every n x n case (k_semi_inverse_reg / k_semi_inverse by width)
        for kind in X.SQUARE_KINDS + X.NONSYM_KINDS:
            A = X.square_case(kind, n, p)
            ctx.set_small(blz.VTAV, np.array(A, np.uint64))
            npiv, winv, d = ctx.semi_inverse()
            want = expect_semi(A, n, p)
            assert npiv == want[0] and [int(w) for w in winv] == want[1] and [int(w) for w in d] == want[2], kind
        for ri, rows in enumerate(rows_list):
            ctx.set_matrix(tall(rows), False)
            for ki, kind in enumerate(X.BLOCK_KINDS):
                v, Av, pb = (X.block_case(kind, rows, n, p, seed=s) for s in (1, 2, 3))
                ctx.set_block(blz.V, np.array(v, np.uint64))
                ctx.set_block(blz.AV, np.array(Av, np.uint64))
                a, b = ctx.block_dot()
                ea, eb = expect_dot(v, Av, rows, n, p)
                assert [int(w) for w in a] == ea and [int(w) for w in b] == eb, ("dot", rows, kind)
                # coefficients from a rank-deficient (mixed d), an all-(p-1) (rank 1) or a full-rank matrix
                sk = ("rank_half", "all_max", "rank_full")[(ri + ki) % 3] if n > 1 else "rank_full"
                S, B = X.square_case(sk, n, p, seed=ri), X.square_case("all_max", n, p)
                ctx.set_block(blz.P, np.array(pb, np.uint64))
                ctx.set_small(blz.VTAV, np.array(S, np.uint64))
                ctx.set_small(blz.VTAAV, np.array(B, np.uint64))
                npiv, winv, d = ctx.semi_inverse()
                assert (npiv, [int(w) for w in winv], [int(w) for w in d]) == expect_semi(S, n, p), sk
                ctx.orthogonalize()
                ev, ep = expect_update(v, Av, pb, [int(w) for w in d], S, B, [int(w) for w in winv], rows, n, p)
                assert [int(w) for w in ctx.get_block(blz.V)] == ev, ("update v", rows, kind, sk)
                assert [int(w) for w in ctx.get_block(blz.P)] == ep, ("update p", rows, kind, sk)


@pytest.mark.parametrize("p,n,padded", STEP_CASES,
                         ids=[f"p{p.bit_length()}b{'f' if p == P61 else ''}-n{n}{'' if pd else '-nopad'}-{p % 1000}"
                              for p, n, pd in STEP_CASES])
def test_update_sums_at_the_reducer_bound(monkeypatch, p, n, padded):
    """v = Av = P = all words p-1, vtAv = J + I (full rank: d is all ones), vtAAv = (n+1) J, so c = -winv vtAAv = -J is
    all p-1 and vtAvd = -(J + I): every one of the 2n products of a v' word is (p-1)^2 or (p-1)(p-2), and every one of
    the n products of a p' word is (p-1) times a residue.  An update kernel that lets one product more than chunk into
    a sum gives wrong words at 57 bits (the generic kernel at exact widths 33 / 48 / 63 reduces in mid-row there)."""
    monkeypatch.setenv("BLZ_NO_PAD", "0" if padded else "1")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    rows = 4099
    S = [(2 if i == j else 1) % p for i in range(n) for j in range(n)]
    B = [(n + 1) % p] * (n * n)
    big = np.full(rows * n, p - 1, dtype=np.uint64)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(tall(rows), False)
        for blk in (blz.V, blz.AV, blz.P):
            ctx.set_block(blk, big)
        ctx.set_small(blz.VTAV, np.array(S, np.uint64))
        ctx.set_small(blz.VTAAV, np.array(B, np.uint64))
        npiv, winv, d = ctx.semi_inverse()
        assert (npiv, ints(winv), ints(d)) == expect_semi(S, n, p)
        assert npiv == n or (n + 1) % p == 0
        ctx.orthogonalize()
        one = [p - 1] * n
        ev, ep = X.orthogonalize(one, one, ints(d), S, B, ints(winv), 1, one, n, p)
        if npiv == n:
            assert ev == [2 * n % p] * n                # -1 + n (p-1)^2 + sum_k (p-1)(-S[k][j]) = -1 + n + n + 1
        assert np.array_equal(ctx.get_block(blz.V).reshape(rows, n), np.tile(np.array(ev, np.uint64), (rows, 1)))
        assert np.array_equal(ctx.get_block(blz.P).reshape(rows, n), np.tile(np.array(ep, np.uint64), (rows, 1)))


@pytest.mark.parametrize("p", FULL + EDGE + OTHER[-3:])
def test_one_long_block_per_chunk_class(monkeypatch, p):
    """70001 rows of edge words at n = 8 (and n = 3, padded to 4, at the two fully covered primes): block_dot and the
    update against the oracle."""
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    rows = 70001
    for n in (8, 3) if p in FULL else (8,):
        v, Av, pb = (np.array(X.block_case("edges", rows, n, p, seed=s), np.uint64) for s in (4, 5, 6))
        S, B = X.square_case("rank_half", n, p, seed=9), X.square_case("rank_full", n, p, seed=10)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(tall(rows), False)
            ctx.set_block(blz.V, v)
            ctx.set_block(blz.AV, Av)
            ctx.set_block(blz.P, pb)
            a, b = ctx.block_dot()
            wa, wb = orc.block_dot(rows, Av, v, n, p, omp_threads=8)
            assert np.array_equal(a, wa) and np.array_equal(b, wb), n
            ctx.set_small(blz.VTAV, np.array(S, np.uint64))
            ctx.set_small(blz.VTAAV, np.array(B, np.uint64))
            npiv, winv, d = ctx.semi_inverse()
            assert 0 < npiv < n or n == 1
            ctx.orthogonalize()
            wv, wp = orc.orthogonalize(v, pb, d, S, B, winv, rows, Av, n, p)
            assert np.array_equal(ctx.get_block(blz.V), wv) and np.array_equal(ctx.get_block(blz.P), wp), n


def dot_lanes(n, padded):
    """Upper bound on the accumulators a stand-alone block_dot spreads the rows over (dot_dispatch, with at most
    num_cu * 8 workgroups): lane groups of the fast kernel, wavefronts of k_block_dot_64, row slices of k_block_dot."""
    w = pow2(n) if padded else n
    cus = device_cus()
    blocks = cus * 8
    if w == 64:
        return min(blocks // 4, cus * 2) * 4
    if w in (1, 2, 4, 8, 16, 32):
        return blocks * (256 // w)
    pairs = w * w
    return blocks * (256 // pairs if pairs <= 256 else 1)


LONG_CASES = [(P57, n, True) for n in (1, 2, 4, 8, 16, 32, 64)] + [(P57, n, False) for n in EXACT_WIDTHS] + \
             [(p, n, True) for p in EDGE + (P61,) for n in (8, 64)]


@pytest.mark.parametrize("p,n,padded", LONG_CASES,
                         ids=[f"p{p.bit_length()}b{'f' if p == P61 else ''}-n{n}{'' if pd else '-nopad'}" for p, n, pd in LONG_CASES])
def test_inner_products_past_chunk_products_per_accumulator(monkeypatch, p, n, padded):
    """v = Av = all words p-1 on enough rows that every accumulator of the launch takes at least chunk + 2 products
    between the first reduction and the last: both products are then rows mod p in every entry.  An accumulator that
    took one product more than make_modp allows gives wrong words at 57 bits (no slack), two more at 58 to 62."""
    monkeypatch.setenv("BLZ_NO_PAD", "0" if padded else "1")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_NO_MFMA", "1")
    rows = (X.chunk(p) + 2) * dot_lanes(n, padded) + 1
    assert rows * n * 8 * 4 < 2.5e9
    big = np.full(rows * n, p - 1, dtype=np.uint64)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(tall(rows), False)
        ctx.set_block(blz.V, big)
        ctx.set_block(blz.AV, big)
        del big
        a, b = ctx.block_dot()
    assert (a == rows % p).all() and (b == rows % p).all(), (rows, np.unique(a)[:4], np.unique(b)[:4])


# ------------------------------------------------------------------------------------------------ C. SpMV


ROW_LENGTHS = (1, 3, 4, 5, 63, 64, 65, 4096, 4097, 20000)


def bound_matrix(p):
    """Rows of every length in ROW_LENGTHS over disjoint columns, and -- in their own rows and columns -- columns of
    every length, so that both M x and M^T x meet every length; every value 2^32-1 mod p."""
    ii, jj, col = [], [], 0
    for r, L in enumerate(ROW_LENGTHS):
        ii.append(np.full(L, r, dtype=np.int64))
        jj.append(np.arange(col, col + L, dtype=np.int64))
        col += L
    row = len(ROW_LENGTHS)
    for c, L in enumerate(ROW_LENGTHS):
        ii.append(np.arange(row, row + L, dtype=np.int64))
        jj.append(np.full(L, col + c, dtype=np.int64))
        row += L
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    nrows, ncols = row + 3, col + len(ROW_LENGTHS) + 3          # and a few empty rows and columns
    return blz.Matrix(nrows, ncols, ii, jj, np.full(len(ii), X.bound_value(p), dtype=np.uint64).astype(np.uint32))


SPMV_CASES = [(p, n) for p in FULL for n in (1, 8, 16, 64)] + \
             [(p, (1, 8, 16, 64)[i % 4]) for i, p in enumerate(q for q in LADDER if q not in FULL)]


@pytest.mark.parametrize("stage", ["BLZ_STAGE_ALWAYS", "BLZ_NO_STAGE"])
@pytest.mark.parametrize("p,n", SPMV_CASES, ids=[f"p{p}-n{n}" for p, n in SPMV_CASES])
def test_spmv_at_the_bounds(monkeypatch, p, n, stage):
    monkeypatch.setenv(stage, "1")
    M = bound_matrix(p)
    term = X.bound_value(p) * (p - 1)
    assert term % p
    for right in (False, True):
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(M, right)
            for transpose, src, dst in ((right, blz.TMP, blz.AV), (not right, blz.V, blz.TMP)):
                ctx.set_block(src, np.full(ctx.rows(src) * n, p - 1, dtype=np.uint64))
                ctx.spmv(transpose, src, dst)
                counts = np.bincount(M.j if transpose else M.i, minlength=M.ncols if transpose else M.nrows)
                want = np.repeat(np.array([int(c) * term % p for c in counts], dtype=np.uint64), n)
                assert np.array_equal(ctx.get_block(dst), want), (right, transpose)


# ------------------------------------------------------------------------------------------------ D. kernel basis, ranks


KB_PRIMES = tuple(X.largest_prime_below(1 << k) for k in (57, 58, 59, 60)) + (X.largest_prime_below(P61),
                                                                             X.largest_prime_below(1 << 62))
KB_WIDTHS = (2, 5, 12, 24, 32, 48)          # test_gpu_kernel_basis.py covers 1, 3, 4, 8, 16, 64


def ones_echelon(n, p):
    """(p-1) times the rows of [I_(n-1) | 1], then (p-1) times their sum.  The RREF has 1 in every free word of every
    row, so a later row whose pivot words are all p-1 is reduced (k_rref's tile pass) by n-1 products of (p-1)^2 per
    word; as TMP of kernel_basis it makes the null vector (p-1, ..., p-1, 1), and V = all p-1 times it is a sum of
    n-1 products of (p-1)^2 per word (k_block_mul)."""
    rows = [[p - 1 if c in (i, n - 1) else 0 for c in range(n)] for i in range(n - 1)]
    return rows + [[p - 1] * (n - 1) + [(n - 1) * (p - 1) % p]]


@pytest.mark.parametrize("padded", [True, False], ids=["padded", "exact"])
@pytest.mark.parametrize("n", KB_WIDTHS)
@pytest.mark.parametrize("p", KB_PRIMES, ids=[f"p{p.bit_length()}b-{p % 1000}" for p in KB_PRIMES])
def test_block_rref_and_kernel_basis_at_barrett_primes(monkeypatch, p, n, padded):
    monkeypatch.setenv("BLZ_NO_PAD", "0" if padded else "1")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    tile = 4 * 8 * (64 // pow2(n))              # rows of a k_rref tile (4 wavefronts, RREF_U = 8 rows per lane group)
    rows = tile * 2 * device_cus() * 3 + 5      # three tiles for every workgroup of the partial pass and a few more
    cols = 2 * n + 3
    M = blz.Matrix(rows, cols, [0, rows - 1], [0, cols - 1], [1, 1])
    pattern = ones_echelon(n, p)
    pattern = pattern[:-1] + [pattern[-1]] * (n - 1)  # the sum row as often as the echelon rows
    with blz.Context(p, n) as c:
        c.set_matrix(M, False)
        for uniq in ([[p - 1] * n], pattern):       # all words p-1 (rank 1); the echelon and its sum (rank n-1)
            V = np.tile(np.array(uniq, dtype=np.uint64), (rows // len(uniq) + 1, 1))[:rows]
            c.set_block(blz.V, V.reshape(-1))
            E, r, piv = c.block_rref(blz.V)
            W, wr, wpiv = kb.rref(uniq, p, n)       # the row space of the distinct rows is the block's
            assert (r, piv) == (wr, list(wpiv)), uniq[:2]
            assert np.array_equal(E, np.array([[int(w) for w in row] for row in W], dtype=np.uint64))
        # kernel basis: TMP of rank n-1 from the echelon, V = all words p-1
        T = [pattern[i % len(pattern)] for i in range(cols)]
        c.set_block(blz.TMP, np.array(T, dtype=np.uint64).reshape(-1))
        c.set_block(blz.V, np.full(rows * n, p - 1, dtype=np.uint64))
        want = kb.kernel_basis([[p - 1] * n], T, p, n)
        k, z = c.kernel_basis()
        assert k == want["k"] and want["s"] == n - 1
        assert np.array_equal(z, np.array(want["z"].tolist(), dtype=np.uint64))
        got = c.get_block(blz.V).reshape(rows, n)
        row = np.array([int(w) for w in want["basis"][0]], dtype=np.uint64) if k else np.zeros(0, np.uint64)
        assert np.array_equal(got[:, :k], np.tile(row, (rows, 1)))
        assert not got[:, k:].any()


def test_all_reduce_edge_of_nranks_times_p():
    """The ranks all-reduce u64 residues: nranks * p <= 2^64 is required (blz_set_matrix).  At 2^62-57 four loopback
    ranks reproduce the exact wide120x260 trajectory's end; five are refused with EINVAL."""
    from test_gpu_loopback import loopback_solve, together
    path = [q for q in EXACT if "_wide_" in q][0]
    g = np.load(path)
    p, n, right = int(g["prime"]), int(g["n"]), bool(g["right"])
    assert p == (1 << 62) - 57 and 4 * p <= 1 << 64 < 5 * p
    M = fixture_matrix(g, p)
    got = loopback_solve(M, p, n, right, 4, batch=7, extra=5)
    assert all(q["its"] == int(g["iterations"]) for q in got)
    for key in ("v", "p", "tmp"):
        assert np.array_equal(together(got, key), g["final_" + key]), key
    group = blz.LoopGroup(5)
    try:
        with blz.Context(p, n) as ctx:
            ctx.comm_init_loopback(group, 0)
            with pytest.raises(blz.BlzError) as e:
                ctx.set_matrix(M, right, 0, 5)
            assert e.value.code == blz.EINVAL and "2**64" in str(e.value)
    finally:
        group.close()
