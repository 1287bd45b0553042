"""Solves with a right-hand side restated in plain Python integers: the bordered operator written out.

M x = b (right) is the search for a kernel vector of M' = [M | b] whose last coordinate is not zero; x M = b (left)
the same for M' = [M ; b].  The library keeps b OUT of the matrix (its values are 32-bit) and applies it as a dense
border behind each product; here M' is simply built, border entries as Python integers below p < 2^62, and handed to
exact_ref's spmv / iteration / trajectory, whose Coo holds values as int64 and computes with Python `int`.

    augmented        the triplets of M' (the border column / row last; zero entries of b left out)
    planted          a seeded x0 and b = M x0 resp. x0 M
    random_rhs       a seeded b with no relation to M (an inconsistent system where M has more rows than rank)
    residual         M x - b resp. x M - b
    solve            Gaussian elimination mod p: (rank of M, one solution or None, is it the only one)
    from_kernel      the solution a kernel vector of M' with a non-zero last word stands for
"""
import random

import numpy as np

import exact_ref as X


def augmented(M, b, right):
    """exact_ref.Coo of [M | b] (right: one more column) or [M ; b] (one more row)."""
    b = [int(w) for w in b]
    assert len(b) == (M.nrows if right else M.ncols)
    nz = [r for r, w in enumerate(b) if w]
    if right:
        ii, jj = list(M.i) + nz, list(M.j) + [M.ncols] * len(nz)
        return X.Coo(M.nrows, M.ncols + 1, ii, jj, list(M.x) + [b[r] for r in nz])
    ii, jj = list(M.i) + [M.nrows] * len(nz), list(M.j) + nz
    return X.Coo(M.nrows + 1, M.ncols, ii, jj, list(M.x) + [b[r] for r in nz])


def apply(M, x, right, p):
    """M x (right) or x M as a list of residues."""
    return X.spmv(M, [int(w) for w in x], not right, 1, p)


def planted(M, right, p, seed):
    """(x0, b): x0 seeded and uniform below p, b = M x0 (right) or x0 M."""
    rnd = random.Random(0x5EED0000 + seed)
    x0 = [rnd.randrange(p) for _ in range(M.ncols if right else M.nrows)]
    return x0, apply(M, x0, right, p)


def random_rhs(M, right, p, seed):
    rnd = random.Random(0xB0B0000 + seed)
    return [rnd.randrange(p) for _ in range(M.nrows if right else M.ncols)]


def residual(M, x, b, right, p):
    return [(y - int(w)) % p for y, w in zip(apply(M, x, right, p), b)]


def from_kernel(v, p):
    """x with M x = b from a kernel vector v = (y, w) of M', w != 0: M y + w b = 0, so x = -y / w."""
    v = [int(w) for w in v]
    s = (-pow(v[-1], -1, p)) % p
    return [y * s % p for y in v[:-1]]


def solve(M, b, right, p):
    """Gauss-Jordan on the dense system mod p.  Returns (rank, x, unique): x = the solution with every free unknown 0,
    or None when the system is inconsistent; unique = the rank equals the number of unknowns."""
    rows, cols = (M.nrows, M.ncols) if right else (M.ncols, M.nrows)       # equations x unknowns
    A = [[0] * (cols + 1) for _ in range(rows)]
    for i, j, x in zip(M.i, M.j, M.x):
        r, c = (int(i), int(j)) if right else (int(j), int(i))
        A[r][c] = (A[r][c] + int(x)) % p
    for r in range(rows):
        A[r][cols] = int(b[r]) % p
    piv, r = [], 0
    for c in range(cols):
        q = next((k for k in range(r, rows) if A[k][c]), None)
        if q is None:
            continue
        A[r], A[q] = A[q], A[r]
        inv = pow(A[r][c], -1, p)
        A[r] = [w * inv % p for w in A[r]]
        for k in range(rows):
            if k != r and A[k][c]:
                f = A[k][c]
                A[k] = [(a - f * t) % p for a, t in zip(A[k], A[r])]
        piv.append(c)
        r += 1
        if r == rows:
            break
    rank = len(piv)
    if any(A[k][cols] for k in range(rank, rows)):
        return rank, None, False
    x = [0] * cols
    for k, c in enumerate(piv):
        x[c] = A[k][cols]
    return rank, x, rank == cols


def init_v(M, right, n, p):
    """The start of a bordered solve: the reference's stream over the original rows of side 0 with the border row last,
    i.e. the augmented matrix's own start."""
    return X.init_v((M.ncols if right else M.nrows) + 1, n, p)


def as_u64(a):
    return np.array([int(w) for w in a], dtype=np.uint64)
