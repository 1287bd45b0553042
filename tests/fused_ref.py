"""Closed-form expectations for one iteration's products, in plain Python integers.

Independent of the kernels, of the C oracle and of exact_ref: nothing here multiplies a matrix by a block.

Let A be the matrix whose rows are the output rows of the iteration's SECOND product (the one that carries the fused
inner products): tmp = A^T v, Av = A tmp.  A has small non-negative integer values.  With every row of v equal to one
row (o_0 ... o_(n-1)) -- operand("ramp"): o_k = p - (1 + k); operand("max"): o_k = p - 1 -- and, as ordinary integers,

    w = A^T 1   (w_t = sum of column t)          s = A w   (s_c = sum_t A[c,t] w_t)

every word follows from s alone:

    tmp[t,k]    = o_k w_t                         mod p
    Av[c,k]     = o_k s_c                         mod p
    vtAv [i][j] = o_i o_j sum_c s_c               mod p      (sum_c s_c = sum_t w_t^2)
    vtAAv[i][j] = o_i o_j sum_c s_c^2             mod p

With the ramp every entry of the two n x n matrices differs from its neighbours (a wrong mirror or rotation shows), the
totals count every entry of A exactly once (a row dropped or taken twice shows), and for n max s_c < 2^40 every word of
v and every non-zero word of Av is within a factor 1 - 2^-16 of p at primes of 56 bits and more, so sums of them
overflow a reducer as sums of (p-1)^2 would.

as_matrix(A, right) gives the blz.Matrix-style triplets of M: A itself for a left kernel (right = False: the second
product is M tmp), its transpose for a right kernel (M^T tmp).

Builders (all return a Coo with .nrows, .ncols, .i, .j, .x of A):
    perm      one entry per row and column
    ladder    rows of prescribed lengths over disjoint columns
    hot       every row also reads a few shared columns (the renumbering then plans an LDS panel)
    band      rows reading neighbouring columns (gathers that hit)
    mixed     concatenation of pieces on disjoint rows and columns
Values: "ones", "palette" (at most 256 distinct small values), "array" (more than 256 distinct small values).
"""
import numpy as np

S_LIMIT = 1 << 40          # n * max s_c stays below this: int64 sums are exact and every word is near p


class Coo:
    def __init__(self, nrows, ncols, i, j, x):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.i = np.ascontiguousarray(i, dtype=np.int64)
        self.j = np.ascontiguousarray(j, dtype=np.int64)
        self.x = np.ascontiguousarray(x, dtype=np.int64)
        self.nnz = len(self.i)
        assert len(self.j) == self.nnz and len(self.x) == self.nnz


# ------------------------------------------------------------------------------------------------ values


def values(count, mode, seed=0):
    """`count` small positive integers.  ones: all 1; palette: 1 ... 200 (fits the packed stream's 256-entry palette);
    array: 1 ... 1000, with every value present when count allows (more than 256 distinct: a separate value array)."""
    if mode == "ones":
        return np.ones(count, dtype=np.int64)
    rng = np.random.default_rng([seed, count, 0x76616C])
    if mode == "palette":
        return rng.integers(1, 201, size=count, dtype=np.int64)
    if mode == "array":
        x = rng.integers(1, 1001, size=count, dtype=np.int64)
        k = min(count, 1000)
        x[:k] = np.arange(1, k + 1)
        return x
    raise ValueError(mode)


# ------------------------------------------------------------------------------------------------ builders


def perm(R, seed=None, mode="ones"):
    """R x R, one entry per row and column: the identity (seed None) or a seeded random permutation."""
    i = np.arange(R, dtype=np.int64)
    j = i.copy() if seed is None else np.random.default_rng([seed, R]).permutation(R).astype(np.int64)
    return Coo(R, R, i, j, values(R, mode, seed or 0))


def ladder(lengths, repeat=1, mode="ones", seed=0):
    """Row r has lengths[r % len(lengths)] entries (the list repeated `repeat` times), over columns no other row
    reads; two empty rows and two empty columns at the end."""
    L = np.tile(np.asarray(lengths, dtype=np.int64), repeat)
    nnz = int(L.sum())
    i = np.repeat(np.arange(len(L), dtype=np.int64), L)
    j = np.arange(nnz, dtype=np.int64)
    return Coo(len(L) + 2, nnz + 2, i, j, values(nnz, mode, seed))


def hot(R, T, per_row, hot_cols, mode="ones", seed=0):
    """R x T: every row reads `per_row` seeded random columns among the last T - hot_cols and two of the first
    `hot_cols` ones (row r: r % hot_cols and (7 r + 3) % hot_cols), so the hot columns hold 2 / (per_row + 2) of the
    entries.  A repeated (row, column) pair is kept: duplicates are summed by the closed form as the SpMV does."""
    rng = np.random.default_rng([seed, R, T, per_row, hot_cols])
    r = np.arange(R, dtype=np.int64)
    cold = rng.integers(hot_cols, T, size=(R, per_row), dtype=np.int64)
    j = np.concatenate([cold, (r % hot_cols)[:, None], ((7 * r + 3) % hot_cols)[:, None]], axis=1).reshape(-1)
    i = np.repeat(r, per_row + 2)
    return Coo(R, T, i, j, values(len(i), mode, seed))


def band(R, per_row, mode="ones", seed=0):
    """R x R: row r reads columns r, r + 1, ..., r + per_row - 1 (mod R)."""
    r = np.arange(R, dtype=np.int64)
    j = ((r[:, None] + np.arange(per_row, dtype=np.int64)[None, :]) % R).reshape(-1)
    return Coo(R, R, np.repeat(r, per_row), j, values(R * per_row, mode, seed))


def mixed(parts):
    """The pieces on disjoint rows and columns of one matrix (block diagonal), rows in the order given."""
    ii, jj, xx, r0, c0 = [], [], [], 0, 0
    for a in parts:
        ii.append(a.i + r0)
        jj.append(a.j + c0)
        xx.append(a.x)
        r0 += a.nrows
        c0 += a.ncols
    return Coo(r0, c0, np.concatenate(ii), np.concatenate(jj), np.concatenate(xx))


def shuffled_rows(A, seed):
    """The same matrix with its rows in a seeded random order (the lists of long rows then interleave with the rest)."""
    q = np.random.default_rng([seed, A.nrows]).permutation(A.nrows).astype(np.int64)
    return Coo(A.nrows, A.ncols, q[A.i], A.j, A.x)


def as_matrix(A, right):
    """(nrows, ncols, i, j, x) of M: A for a left kernel, A^T for a right kernel."""
    if right:
        return A.ncols, A.nrows, A.j, A.i, A.x
    return A.nrows, A.ncols, A.i, A.j, A.x


# ------------------------------------------------------------------------------------------------ the closed form


def operand(kind, n, p):
    """The row every block row of v holds."""
    if kind == "ramp":
        return [(p - (1 + k)) % p for k in range(n)]
    if kind == "max":
        return [p - 1] * n
    raise ValueError(kind)


def column_and_row_sums(A, p, n):
    """(w, s) as int64 arrays; values are taken mod p first (what a matrix loaded at p holds).  Sums of integers below
    2^53 in float64 (np.bincount) are exact."""
    x = A.x % p
    assert int(x.sum()) < 1 << 53
    w = np.bincount(A.j, weights=x, minlength=A.ncols).astype(np.int64)
    xw = x * w[A.j]
    assert int(w.max(initial=0)) * int(x.max(initial=0)) < 1 << 53      # (partial sums never exceed the final, non-negative terms)
    s = np.bincount(A.i, weights=xw, minlength=A.nrows).astype(np.int64)
    assert n * int(s.max(initial=0)) < S_LIMIT, "n * max s_c must stay below 2^40"
    return w, s


def _scaled_rows(s, o, p):
    """The block whose row c is (o_k s_c mod p)_k, flat u64."""
    top = int(s.max(initial=0))
    if all((p - ok) * top < p for ok in o):
        # o_k = p - a with a s_c < p: o_k s_c = -(a s_c) mod p, no reduction needed
        a = np.array([p - ok for ok in o], dtype=np.uint64)
        prod = s.astype(np.uint64)[:, None] * a[None, :]
        return np.where(prod == 0, np.uint64(0), np.uint64(p) - prod).reshape(-1)
    uniq, inv = np.unique(s, return_inverse=True)       # (small matrices at small primes) a table over the distinct s
    table = np.array([[int(u) * int(ok) % p for ok in o] for u in uniq], dtype=np.uint64)
    return table[inv.reshape(-1)].reshape(-1)


def totals(s):
    """(sum_c s_c, sum_c s_c^2) as Python integers: s in three limbs of 13 bits, so that no int64 sum wraps."""
    assert int(s.max(initial=0)) < 1 << 39 and int(s.min(initial=0)) >= 0 and len(s) < 1 << 26
    a, b, c = s >> 26, (s >> 13) & 8191, s & 8191
    dot = lambda u, v: int((u * v).sum())                               # noqa: E731  (terms < 2^26, sums < 2^52)
    t2 = (dot(a, a) << 52) + (dot(a, b) << 40) + ((2 * dot(a, c) + dot(b, b)) << 26) + (dot(b, c) << 14) + dot(c, c)
    return int(s.sum()), t2


def expect(A, n, p, kind):
    """dict(v, tmp, Av: flat u64 blocks; vtAv, vtAAv: flat u64 n x n; sum_s, sum_s2: the integer totals)."""
    o = operand(kind, n, p)
    w, s = column_and_row_sums(A, p, n)
    t1, t2 = totals(s)
    assert t1 == totals(w)[1]
    return dict(v=np.tile(np.array(o, dtype=np.uint64), A.nrows),
                tmp=_scaled_rows(w, o, p), Av=_scaled_rows(s, o, p),
                vtAv=np.array([o[i] * o[j] * t1 % p for i in range(n) for j in range(n)], dtype=np.uint64),
                vtAAv=np.array([o[i] * o[j] * t2 % p for i in range(n) for j in range(n)], dtype=np.uint64),
                sum_s=t1, sum_s2=t2, s=s)


def smallest_words(n, p):
    """Lower bounds of the non-zero words the builders and operands give at n * max s_c < S_LIMIT and p > 2^41:
    (smallest word of v, smallest non-zero word of Av)."""
    assert p > S_LIMIT * 2
    return p - n, p - S_LIMIT
