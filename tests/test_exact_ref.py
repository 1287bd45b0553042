"""The chain reference -> exact integers -> oracle, at every reducer class (no GPU).

1. tests/exact_ref.py (plain Python integers, no oracle, no library) reproduces every fixture the reference itself
   produced (semi_inverse.npz, kern_*.npz, traj_*.npz, p <= 2^31-1): the restatement is the reference's algorithm.
2. At every prime of exact_ref.ladder() -- one or two per bit length from 2 to 62 bits, every chunk class of
   csrc/modp.h -- the oracle equals exact_ref on operands at their bounds: SpMV rows of 2^32-1 mod p times p-1,
   block_dot / semi_inverse / orthogonalize on the seeded edge cases.  From here on the oracle may stand in for exact
   integers where Python is too slow.
3. The oracle reproduces the exact_*.npz fixtures (written by golden/make_exact_golden.py from exact_ref alone), which
   the GPU tests (test_gpu_exact.py) check the kernels against.
"""
import glob
import json
import os

import numpy as np
import pytest

import exact_ref as X
import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAJ = sorted(glob.glob(os.path.join(GOLDEN, "traj_*.npz")))
KERN = sorted(glob.glob(os.path.join(GOLDEN, "kern_*.npz")))
EXACT = sorted(glob.glob(os.path.join(GOLDEN, "exact_*.npz")))
MATRIX_OF = {"tref": "trefethen20", "r300": "rand300x200", "wide": "wide120x260",
             "quirks": "quirks40x30", "r3000": "rand3000x2000"}
LADDER = X.ladder()

# the reducer table: bit length -> (chunk, products of (p-1)^2 plus one residue that fit, at the largest prime below 2^k)
CHUNK_TABLE = {56: (64, 128), 57: (64, 64), 58: (31, 32), 59: (15, 16), 60: (7, 8), "61b": (3, 4), "61f": (32, 64),
               62: (1, 2)}


def ints(a):
    return [int(w) for w in np.asarray(a).reshape(-1)]


def matrix_for(path, p):
    return X.load_mtx(os.path.join(GOLDEN, MATRIX_OF[os.path.basename(path).split("_")[1]] + ".mtx"), p)


def as_orc(M):
    return orc.Matrix(M.nrows, M.ncols, M.i, M.j, M.x)


# ------------------------------------------------------------------------------------------------ ladder and chunk


def test_ladder_covers_every_reducer_class():
    assert all(X.is_prime(p) for p in LADDER)
    assert not any(X.is_prime(q) for q in (1, 561, 3215031751, (1 << 61) - 3, 3825123056546413051))
    bits = {p.bit_length() for p in LADDER}
    assert set(X.LADDER_BITS) <= bits
    for k in X.LADDER_BITS:
        if k == 2:
            continue
        lo, hi = X.smallest_prime_above(1 << (k - 1)), X.largest_prime_below(1 << k)
        assert lo in LADDER and hi in LADDER and lo.bit_length() == hi.bit_length() == k
    assert (1 << 61) - 1 in LADDER and (1 << 31) - 1 in LADDER and (1 << 61) - 31 in LADDER
    # every row of the table is reached, at the prime that makes it tight
    seen = {}
    for p in LADDER:
        k = p.bit_length()
        key = ("61f" if X.reducer(p) == "fold61" else "61b") if k == 61 else k
        if key in CHUNK_TABLE and (key not in seen or p > seen[key][0]):
            seen[key] = (p, X.chunk(p), X.slack(p))
    assert set(seen) == set(CHUNK_TABLE)
    for key, (p, c, s) in seen.items():
        want_c, want_s = CHUNK_TABLE[key]
        assert c == want_c and (s == want_s if key != 56 else s >= want_s), (key, p, c, s)
    # make_modp's promise: a residue plus `chunk` products never passes the reducer's bound
    for p in LADDER:
        assert X.chunk(p) <= X.slack(p), p
    # the kernel choice the table describes (ortho_dispatch: fast n needs chunk >= 2n; _32 / _64 need chunk >= 32)
    assert [n for n in (1, 2, 4, 8, 16) if X.chunk((1 << 59) - 55) >= 2 * n] == [1, 2, 4]


def test_rng_and_loader_match_reference():
    g = json.load(open(os.path.join(GOLDEN, "rng.json")))
    assert X.rng_draws(len(g["draws"])) == g["draws"]
    for a, p, inv in g["invmod"]:
        assert X.invmod(a, p) == inv
    for path in TRAJ:
        t = np.load(path)
        M = matrix_for(path, int(t["prime"]))
        assert ints(M.i) == ints(t["coo_i"]) and ints(M.j) == ints(t["coo_j"]) and ints(M.x) == ints(t["coo_x"])
        assert X.init_v(int(t["nrows"]), int(t["n"]), int(t["prime"])) == ints(t["v0"])


# ------------------------------------------------------------------------------------------------ 1. reference fixtures


def test_semi_inverse_reference_vectors():
    g = np.load(os.path.join(GOLDEN, "semi_inverse.npz"))
    for key in sorted(k[:-2] for k in g.files if k.endswith("_M")):
        n, p = int(key.split("_")[0][1:]), int(key.split("_")[1][1:])
        for M, winv, d, npiv in zip(g[key + "_M"], g[key + "_winv"], g[key + "_d"], g[key + "_npiv"]):
            got = X.semi_inverse(ints(M), n, p)
            assert got == (int(npiv), ints(winv), ints(d)), key


@pytest.mark.parametrize("path", KERN, ids=[os.path.basename(p)[5:-4] for p in KERN])
def test_kernel_steps_reference_vectors(path):
    g = np.load(path)
    p, n, right = int(g["prime"]), int(g["n"]), bool(g["right"])
    M = matrix_for(path, p)
    nrows = M.ncols if right else M.nrows
    for it in sorted({k.split("_")[0] for k in g.files if k.startswith("it")}):
        v, tmp, Av, pb = (ints(g[f"{it}_{k}"]) for k in ("v", "tmp", "Av", "p"))
        assert X.spmv(M, v, not right, n, p) == tmp
        assert X.spmv(M, tmp, right, n, p) == Av
        a, b = X.block_dot(nrows, Av, v, n, p)
        assert a == ints(g[f"{it}_vtAv"]) and b == ints(g[f"{it}_vtAAv"])
        npiv, winv, d = X.semi_inverse(a, n, p)
        assert winv == ints(g[f"{it}_winv"]) and d == ints(g[f"{it}_d"])
        vn, pn = X.orthogonalize(v, pb, d, a, b, winv, nrows, Av, n, p)
        assert vn == ints(g[f"{it}_vnext"]) and pn == ints(g[f"{it}_pnext"])


@pytest.mark.parametrize("path", TRAJ, ids=[os.path.basename(p)[5:-4] for p in TRAJ])
def test_trajectory_reference_vectors(path):
    g = np.load(path)
    p, n, right, stop = int(g["prime"]), int(g["n"]), bool(g["right"]), int(g["stop_after"])
    M = matrix_for(path, p)
    recs, end = X.trajectory(M, n, p, right=right, stop_after=stop)
    assert len(recs) == len(g["npiv"])
    for k, r in enumerate(recs):
        assert r["npiv"] == int(g["npiv"][k]) and X.sha(r["v"]) == str(g["vhash"][k]), k
        for name in ("vtAv", "vtAAv", "winv", "d"):
            assert r[name] == ints(g[name][k]), (name, k)
    assert end["iterations"] == int(g["iterations"]) and end["v"] == ints(g["final_v"])
    if stop <= 0:
        assert end["tmp"] == ints(g["final_tmp"])


# ------------------------------------------------------------------------------------------------ 2. oracle == exact


@pytest.mark.parametrize("p", LADDER)
def test_oracle_spmv_at_the_bounds(p):
    """Rows of 1 ... 5000 entries, every value 2^32-1 mod p (p-1 where that is 0), every operand word p-1:
    y = len * value * (p-1)."""
    lens = [1, 2, 3, 63, 64, 65, 1000, 5000]
    val = X.bound_value(p)
    assert val != 0
    ii = np.concatenate([np.full(L, r, dtype=np.int32) for r, L in enumerate(lens)])
    jj = np.concatenate([np.arange(L, dtype=np.int32) for L in lens])
    M = orc.Matrix(len(lens), 5000, ii, jj, np.full(len(ii), val, dtype=np.uint32))
    for n in (1, 3, 8):
        for right in (False, True):
            rows_in = M.nrows if right else M.ncols
            x = np.full(rows_in * n, p - 1, dtype=np.uint64)
            got = orc.spmv(M, x, right, n, p)
            if right:      # column j collects one entry from every row at least j+1 long
                want = [sum(1 for L in lens if L > j) * val * (p - 1) % p for j in range(5000) for _ in range(n)]
            else:
                want = [L * val * (p - 1) % p for L in lens for _ in range(n)]
            assert ints(got) == want
    y = ints(orc.spmv(M, np.full(5000 * 3, p - 1, dtype=np.uint64), False, 3, p))
    assert y == X.spmv(M, [p - 1] * (5000 * 3), False, 3, p)


def _chunk_class_reps():
    """The largest ladder prime of each chunk value (plus both 61-bit reducers)."""
    reps = {}
    for p in LADDER:
        key = (X.chunk(p), X.reducer(p))
        reps[key] = max(reps.get(key, 0), p)
    return sorted(reps.values())


@pytest.mark.parametrize("p", LADDER)
def test_oracle_dense_steps_equal_exact(p):
    """semi_inverse on every n x n case, block_dot and orthogonalize on every operand kind, n in {1, 2, 3, 8, 16}, and
    n = 64 once per chunk class."""
    widths = [1, 2, 3, 8, 16] + ([64] if p in _chunk_class_reps() else [])
    for n in widths:
        kinds = X.SQUARE_KINDS + (X.NONSYM_KINDS if n in (3, 8) else ())
        if n == 64:
            kinds = ("rank_half", "all_max")
        for kind in kinds:
            A = X.square_case(kind, n, p)
            npiv, winv, d = orc.semi_inverse(np.array(A, dtype=np.uint64), n, p)
            assert (npiv, ints(winv), ints(d)) == X.semi_inverse(A, n, p), (kind, n)
        rows = 37 if n < 64 else 9
        for kind in X.BLOCK_KINDS:
            v, Av, pb = (X.block_case(kind, rows, n, p, seed=s) for s in (1, 2, 3))
            a, b = orc.block_dot(rows, np.array(Av, np.uint64), np.array(v, np.uint64), n, p)
            ea, eb = X.block_dot(rows, Av, v, n, p)
            assert ints(a) == ea and ints(b) == eb, (kind, n)
            # coefficients from a rank-deficient semi_inverse (mixed d) and from a full one
            for sk in (("rank_half", "all_max") if n >= 2 else ("rank_full",)):
                S = X.square_case(sk, n, p, seed=7)
                B = X.square_case("rank_full", n, p, seed=8)
                npiv, winv, d = X.semi_inverse(S, n, p)
                got = orc.orthogonalize(np.array(v, np.uint64), np.array(pb, np.uint64), d, S, B, winv, rows,
                                        np.array(Av, np.uint64), n, p)
                want = X.orthogonalize(v, pb, d, S, B, winv, rows, Av, n, p)
                assert ints(got[0]) == want[0] and ints(got[1]) == want[1], (kind, sk, n)


def test_generators_reach_their_edges():
    p, n = X.largest_prime_below(1 << 57), 16
    assert X.semi_inverse(X.square_case("zero", n, p), n, p)[0] == 0
    for kind, r in (("rank1", 1), ("rank_half", n // 2), ("rank_nm1", n - 1), ("rank_full", n)):
        assert sum(X.phase1_columns(X.square_case(kind, n, p), n, p)) == r, kind
    sel = X.phase1_columns(X.square_case("nonprefix", n, p), n, p)
    assert sel != sorted(sel, reverse=True) and sel[0] == 0
    assert X.phase1_columns(X.square_case("zero_mid", n, p), n, p)[n // 2] == 0
    A = X.square_case("zero_diag", n, p)
    assert all(A[i * n + i] == 0 for i in range(n)) and X.semi_inverse(A, n, p)[0] == n
    e = X.block_case("edges", 4099, 8, p)
    assert e.count(p - 1) >= len(e) // 4 and e.count(0) >= len(e) // 8


# ------------------------------------------------------------------------------------------------ 3. exact fixtures


@pytest.mark.parametrize("path", EXACT, ids=[os.path.basename(p)[6:-4] for p in EXACT])
def test_oracle_reproduces_exact_fixture(path):
    g = np.load(path)
    p, n, right, stop = int(g["prime"]), int(g["n"]), bool(g["right"]), int(g["stop_after"])
    name = str(g["matrix"])
    if name == "synth":
        import blz
        nr, nc, nz, seed = (int(x) for x in g["synth"])
        S = blz.Matrix.synth(nr, nc, nz, seed, p)
        M = orc.Matrix(S.nrows, S.ncols, S.i, S.j, S.x)
    else:
        M = orc.Matrix.load(os.path.join(GOLDEN, name + ".mtx"), p)
    assert X.coo_sha(M.i, M.j, M.x) == str(g["coo_sha"])
    recs = []
    res = orc.block_lanczos(M, n, p, right=right, stop_after=stop, trace=recs.append)
    assert res["iterations"] == int(g["iterations"]) and len(recs) == len(g["npiv"])
    if stop <= 0:
        assert recs[-1]["npiv"] == 0 and g["npiv"][-1] == 0
    for k, r in enumerate(recs):
        assert r["npiv"] == g["npiv"][k] and X.sha(r["v"]) == str(g["vhash"][k]), k
        for key in ("vtAv", "vtAAv", "winv", "d"):
            assert np.array_equal(r[key], g[key][k]), (key, k)
    for key, got in (("v", res["v"]), ("p", res["p"]), ("tmp", res["tmp"])):
        if "final_" + key in g.files:
            assert np.array_equal(got, g["final_" + key]), key
        elif key != "tmp" or stop <= 0:
            assert X.sha(got) == str(g["final_" + key + "_sha"]), key
    assert os.path.getsize(path) <= 256 * 1024


def test_exact_fixtures_fit_their_budget():
    assert len(EXACT) >= 7
    assert sum(os.path.getsize(p) for p in EXACT) <= 1 << 20
    primes = {int(np.load(p)["prime"]).bit_length() for p in EXACT}
    assert {58, 59, 60, 61, 62} <= primes
