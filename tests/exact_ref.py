"""Block Lanczos mod p restated in plain Python integers -- the exact reference the suite compares with.

Nothing here calls the CPU oracle (oracle/) or the library: every word is computed with Python `int` (numpy arrays
of dtype=object where a whole block is handled at once), so sums never wrap and never need a reducer.  The steps
follow the reference's sequential program:

    spmv          y = M x or M^T x, entry by entry (sequential/lanczos_modp.c:280-301)
    block_dot     v^T Av and Av^T Av (:443-453)
    semi_inverse  phase 1 selects the pivot columns on the whole matrix, phase 2 eliminates the masked matrix
                  carrying the identity (:342-438)
    ortho_coeffs  the n x n matrices c = -winv * spliced and vtAvd (:456-475)
    orthogonalize the next v and p (:476-492)
    iteration     one pass of the loop body (:635-656); trajectory() runs it to termination or stop_after

plus the matrix loader's value rule, the seeded initial block (:67-87, :624-625), a deterministic prime ladder
across the reducer classes of csrc/modp.h, and seeded generators of n x n and block operands at their edges.
"""
import hashlib
import random
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------------ primes and chunk


def is_prime(q):
    """Deterministic Miller-Rabin: the bases 2..37 decide every q < 3.3 * 10^24."""
    if q < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in small:
        if q % b == 0:
            return q == b
    d, s = q - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for b in small:
        x = pow(b, d, q)
        if x in (1, q - 1):
            continue
        for _ in range(s - 1):
            x = x * x % q
            if x == q - 1:
                break
        else:
            return False
    return True


LADDER_BITS = (2, 8, 17, 31, 32, 33, 40, 48, 56, 57, 58, 59, 60, 61, 62)
P31, P61 = (1 << 31) - 1, (1 << 61) - 1


def largest_prime_below(x):
    q = x - 1
    while not is_prime(q):
        q -= 1
    return q


def smallest_prime_above(x):
    q = x + 1
    while not is_prime(q):
        q += 1
    return q


def ladder():
    """For every k of LADDER_BITS the largest prime below 2^k and the smallest above 2^(k-1) (both of bit length k),
    plus the two folding primes 2^31-1 and 2^61-1 and the largest Barrett prime below 2^61 (2^61-31: the largest
    below 2^61 is 2^61-1 itself, which folds).  Sorted, without repeats."""
    out = {P31, P61, largest_prime_below(P61)}
    for k in LADDER_BITS:
        out.add(largest_prime_below(1 << k))
        out.add(smallest_prime_above(1 << (k - 1)))
    return sorted(out)


def chunk(p):
    """csrc/modp.h make_modp(): how many products of two residues a dense sum may take before a reduction.
    Barrett (every p but 2^61-1 and 2^31-1) is exact for T < 2^(63+k), k = bit length of p, and a sum is a residue
    plus chunk products: chunk = 64 while 63 - k >= 6, else 2^(63-k) - 1 (at least 1).  Folding at 2^61-1 takes any
    128-bit value: 32.  2^31-1 folds too but keeps the Barrett count (its words are 32-bit)."""
    k = p.bit_length()
    room = 63 - k
    c = 64 if room >= 6 else max((1 << room) - 1, 1)
    return 32 if p == P61 else c


def reducer(p):
    """'fold61', 'fold31' or 'barrett' (modp_mersenne)."""
    return "fold61" if p == P61 else ("fold31" if p == P31 else "barrett")


def bound_value(p):
    """The largest matrix value the loader can give at p: 2^32-1 mod p, or p-1 where p divides 2^32-1
    (= 3 * 5 * 17 * 257 * 65537) and that residue would be 0."""
    v = (2 ** 32 - 1) % p
    return v if v else p - 1


def slack(p):
    """How many products of (p-1)^2, plus one residue, still fit the reducer's bound (2^(63+k), or 2^128 folding)."""
    bound = 1 << 128 if p == P61 else 1 << (63 + p.bit_length())
    return (bound - p) // ((p - 1) ** 2) if p > 2 else (bound - p)


# ------------------------------------------------------------------------------------------------ matrix and RNG


class Coo:
    """COO triplets in file order, values already reduced mod p (the reference's sparsematrix_t)."""

    def __init__(self, nrows, ncols, i, j, x):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.i = np.asarray(i, dtype=np.int64)
        self.j = np.asarray(j, dtype=np.int64)
        self.x = np.asarray(x, dtype=np.int64)
        self.nnz = len(self.i)


def load_mtx(path, p):
    """MatrixMarket coordinate integer general.  A value is scanned as a signed int and stored as u32, so a negative
    entry wraps to 2^32 - |x| BEFORE the reduction mod p (sequential/lanczos_modp.c:238-243)."""
    with open(path) as f:
        lines = [ln for ln in f if not ln.startswith("%")]
    nr, nc, nz = (int(t) for t in lines[0].split())
    ii, jj, xx = [], [], []
    for ln in lines[1:1 + nz]:
        a, b, c = ln.split()
        ii.append(int(a) - 1)
        jj.append(int(b) - 1)
        xx.append((int(c) & 0xFFFFFFFF) % p)
    return Coo(nr, nc, ii, jj, xx)


def rng_draws(count):
    """The reference's generator (sequential/lanczos_modp.c:67, :76-87): four fixed seed words, output
    rotl(s0 + s3, 23) + s0, xoshiro256 transition with shift 17 and rotation 45."""
    mask = (1 << 64) - 1

    def rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & mask

    s = [0x1415926535, 0x8979323846, 0x2643383279, 0x5028841971]
    out = []
    for _ in range(count):
        out.append((rotl((s[0] + s[3]) & mask, 23) + s[0]) & mask)
        carry = (s[1] << 17) & mask
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= carry
        s[3] = rotl(s[3], 45)
    return out


def init_v(nrows, n, p):
    """The initial block: one draw per word in row-major order, reduced mod p (:624-625)."""
    return [w % p for w in rng_draws(nrows * n)]


# ------------------------------------------------------------------------------------------------ the steps


def _obj(a, cols):
    return np.array([int(w) for w in a], dtype=object).reshape(-1, cols)


def _flat(A, p):
    return [int(w) % p for w in np.asarray(A, dtype=object).reshape(-1)]


def spmv(M, x, transpose, n, p):
    """y = M x (transpose=False) or M^T x, x and y row-major blocks of width n."""
    rows_out = M.ncols if transpose else M.nrows
    X = _obj(x, n)
    r, c = (M.j, M.i) if transpose else (M.i, M.j)
    Y = np.zeros((rows_out, n), dtype=object)
    Y[:] = 0
    if M.nnz:
        vals = np.array([int(a) for a in M.x], dtype=object)[:, None]
        np.add.at(Y, r, X[c] * vals)
    return _flat(Y, p)


def block_dot(N, Av, v, n, p):
    """(v^T Av, Av^T Av) over the first N block rows, n x n row-major."""
    Vb, Ab = _obj(v, n)[:N], _obj(Av, n)[:N]
    return _flat(Vb.T.dot(Ab), p), _flat(Ab.T.dot(Ab), p)


def invmod(a, p):
    return pow(int(a), -1, int(p))


def _sweep(a, w, d, n, p):
    """One Gauss-Jordan pass over the columns (the reference's "dance"): on column j the first row i >= j with a
    non-zero entry is scaled to a unit pivot and swapped into row j, then column j is cleared in every other row.
    Columns without such a row are skipped.  w, if given, undergoes the same row operations."""
    cnt = 0
    for j in range(n):
        piv = next((i for i in range(j, n) if a[i * n + j] != 0), None)
        if piv is None:
            continue
        d[j] = 1
        cnt += 1
        inv = invmod(a[piv * n + j], p)
        for k in range(n):
            a[piv * n + k] = a[piv * n + k] * inv % p
            if w is not None:
                w[piv * n + k] = w[piv * n + k] * inv % p
        for k in range(n):
            a[j * n + k], a[piv * n + k] = a[piv * n + k], a[j * n + k]
            if w is not None:
                w[j * n + k], w[piv * n + k] = w[piv * n + k], w[j * n + k]
        for i in range(n):
            if i == j:
                continue
            m = a[i * n + j]
            if m == 0:
                continue
            for k in range(n):
                a[i * n + k] = (a[i * n + k] - m * a[j * n + k]) % p
                if w is not None:
                    w[i * n + k] = (w[i * n + k] - m * w[j * n + k]) % p
    return cnt


def semi_inverse(M_, n, p):
    """(npiv, winv, d) with d W = W d = W and d = W M d (sequential/lanczos_modp.c:342-438).  Phase 1 selects the
    columns d on the whole matrix; phase 2 restarts on M masked to the selected rows and columns, carrying the
    identity restricted to them, and its own pivot set is the d returned."""
    M_ = [int(w) for w in M_]
    sel = [0] * n
    _sweep(list(M_), None, sel, n, p)
    a = [M_[i * n + j] if sel[i] and sel[j] else 0 for i in range(n) for j in range(n)]
    w = [1 if i == j and sel[i] else 0 for i in range(n) for j in range(n)]
    d = [0] * n
    return _sweep(a, w, d, n, p), w, d


def phase1_columns(M_, n, p):
    """The columns phase 1 of semi_inverse selects."""
    sel = [0] * n
    _sweep([int(w) for w in M_], None, sel, n, p)
    return sel


def ortho_coeffs(vtAv, vtAAv, winv, d, n, p):
    """(c, vtAvd): c = -winv * spliced, spliced[i][j] = d[j] ? vtAAv[i][j] : vtAv[i][j]; vtAvd[i][j] = d[j] ? -vtAv[i][j]
    : 0 (:456-475).  Canonical residues (the reference leaves p for 0 here; the sums it feeds are the same mod p)."""
    A, B, W = (_obj(x, n) for x in (vtAv, vtAAv, winv))
    dm = np.array([bool(int(x)) for x in d])
    spl = np.where(dm[None, :], B, A)
    c = _flat(-W.dot(spl), p)
    vd = _flat(np.where(dm[None, :], -A, 0), p)
    return c, vd


def orthogonalize(v, pb, d, vtAv, vtAAv, winv, N, Av, n, p):
    """(v_next, p_next) for the first N block rows (:476-492):
        v'[r,j] = (d[j] ? Av[r,j] : v[r,j]) + sum_k v[r,k] c[k,j] + sum_k p[r,k] vtAvd[k,j]
        p'[r,j] = (d[j] ? 0 : p[r,j]) + sum_k v[r,k] winv[k,j]"""
    c, vd = ortho_coeffs(vtAv, vtAAv, winv, d, n, p)
    Vb, Ab, Pb = _obj(v, n)[:N], _obj(Av, n)[:N], _obj(pb, n)[:N]
    C_, VD, W = _obj(c, n), _obj(vd, n), _obj(winv, n)
    dm = np.array([bool(int(x)) for x in d])
    nv = np.where(dm[None, :], Ab, Vb) + Vb.dot(C_) + Pb.dot(VD)
    npb = np.where(dm[None, :], 0, Pb) + Vb.dot(W)
    return _flat(nv, p), _flat(npb, p)


def iteration(M, n, p, right, v, pb):
    """One pass of the loop body.  Returns (npiv, v_next, p_next, tmp, (vtAv, vtAAv, winv, d)); when npiv == 0 the
    loop stops and v, p are returned unchanged."""
    nrows = M.ncols if right else M.nrows
    tmp = spmv(M, v, not right, n, p)
    Av = spmv(M, tmp, right, n, p)
    vtAv, vtAAv = block_dot(nrows, Av, v, n, p)
    npiv, winv, d = semi_inverse(vtAv, n, p)
    if npiv == 0:
        return npiv, list(v), list(pb), tmp, (vtAv, vtAAv, winv, d)
    nv, npb = orthogonalize(v, pb, d, vtAv, vtAAv, winv, nrows, Av, n, p)
    return npiv, nv, npb, tmp, (vtAv, vtAAv, winv, d)


def trajectory(M, n, p, right=False, stop_after=-1, v0=None):
    """Runs iteration() from init_v (or v0) until npiv == 0 or stop_after iterations.  Returns (records, end): one
    record per iteration evaluated (v before it, vtAv, vtAAv, winv, d, npiv, tmp) and end = dict(v, p, tmp,
    iterations).  end["tmp"] is the last record's tmp -- what the reference leaves there on termination."""
    nrows = M.ncols if right else M.nrows
    v = list(v0) if v0 is not None else init_v(nrows, n, p)
    pb = [0] * (nrows * n)
    recs, tmp, it = [], None, 0
    while not (stop_after > 0 and it == stop_after):
        npiv, nv, npb, tmp, (vtAv, vtAAv, winv, d) = iteration(M, n, p, right, v, pb)
        recs.append(dict(v=v, vtAv=vtAv, vtAAv=vtAAv, winv=winv, d=d, npiv=npiv, tmp=tmp))
        if npiv == 0:
            break
        v, pb, it = nv, npb, it + 1
    return recs, dict(v=v, p=pb, tmp=tmp, iterations=it)


def coo_sha(i, j, x):
    """sha256 of a matrix's triplets (each as little-endian int64), to pin a generated matrix."""
    h = hashlib.sha256()
    for a in (i, j, x):
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    return h.hexdigest()


def sha(words):
    """sha256 of a block as little-endian u64 words (the fixtures' vhash)."""
    return hashlib.sha256(np.array([int(w) for w in words], dtype=np.uint64).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ case generators

SQUARE_KINDS = ("zero", "rank1", "rank_half", "rank_nm1", "rank_full", "zero_mid", "zero_diag", "all_max",
                "nonprefix")
NONSYM_KINDS = ("nonsym", "nonsym_zero_diag")


def _bbt(B, n, p):
    """B B^T mod p for an n x r matrix B (list of rows)."""
    return [sum(B[i][t] * B[j][t] for t in range(len(B[i]))) % p for i in range(n) for j in range(n)]


def square_case(kind, n, p, seed=0):
    """Seeded n x n input of semi_inverse (row-major list).  The symmetric kinds are what the solver meets
    (v^T A v is symmetric); the NONSYM_KINDS only reach the stand-alone call."""
    rnd = random.Random(f"{kind}:{n}:{p}:{seed}")
    R = lambda: rnd.randrange(p)                                         # noqa: E731
    if kind == "zero":
        return [0] * (n * n)
    if kind.startswith("rank"):
        r = {"rank1": 1, "rank_half": n // 2, "rank_nm1": n - 1, "rank_full": n}[kind]
        B = [[R() for _ in range(r)] for _ in range(n)]
        return _bbt(B, n, p)
    if kind == "zero_mid":                     # row and column n//2 zero, the rest B B^T of full rank elsewhere
        B = [[R() for _ in range(n)] for _ in range(n)]
        B[n // 2] = [0] * n
        return _bbt(B, n, p)
    if kind == "zero_diag":                    # symmetric, zero diagonal, non-zero off the diagonal: swaps
        a = [0] * (n * n)
        for i in range(n):
            for j in range(i + 1, n):
                a[i * n + j] = a[j * n + i] = R() or 1
        return a
    if kind == "all_max":
        return [p - 1] * (n * n)
    if kind == "nonprefix":                    # phase 1 skips column 0 and every other one after it
        B = [[R() for _ in range(n)] for _ in range(n)]
        for i in range(0, n, 2):
            B[i] = [0] * n
        a = _bbt(B, n, p)
        return a
    if kind == "nonsym":
        return [R() for _ in range(n * n)]
    if kind == "nonsym_zero_diag":
        a = [R() for _ in range(n * n)]
        for i in range(n):
            a[i * n + i] = 0
        if n > 1:
            a[0 * n + 1] = 0                   # row 0 has no pivot on column 1 either: the search goes further down
        return a
    raise ValueError(kind)


BLOCK_KINDS = ("max", "edges", "same_rows")


def block_case(kind, rows, n, p, seed=0):
    """Seeded rows x n block (flat list).  max: every word p-1.  edges: uniform residues with at least a quarter of the
    words at p-1 and an eighth at 0.  same_rows: one random row repeated, so a single exact row stands for all."""
    rng = np.random.default_rng([zlib.crc32(kind.encode()), rows, n, p % (1 << 32), p >> 32, seed])
    if kind == "max":
        return [p - 1] * (rows * n)
    if kind == "edges":
        w = rng.integers(0, p, size=rows * n, dtype=np.uint64)
        at = rng.permutation(rows * n)
        q = -(-rows * n // 4)
        w[at[:q]] = p - 1
        w[at[q:q + -(-rows * n // 8)]] = 0
        return w.tolist()
    if kind == "same_rows":
        return rng.integers(0, p, size=n, dtype=np.uint64).tolist() * rows
    raise ValueError(kind)
