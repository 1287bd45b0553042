"""Helpers of the signed value mode's tests: matrices with signed int32 entries, their files, and expectations in plain
Python integers.  Nothing here calls the library.

In signed value mode an entry a (any int32) means the residue a mod p.  Two references:
  (a) exact_ref's spmv / iteration / trajectory fed a Coo whose values are a % p as Python ints (residues());
  (b) a closed form: when every block row of the operand is the same row o, y[r, k] = (s_r mod p) * o_k mod p with s_r
      the SIGNED integer sum of row r (np.bincount on int64, exact below 2^53 -- asserted).
"""
import numpy as np

import exact_ref as X
import fused_ref as F

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def signed_values(count, mode, seed=0):
    """palette: +-1 ... +-100 (at most 200 distinct values: the packed stream); array: +-1 ... +-1000 with INT32_MIN,
    INT32_MAX and -1 each present (more than 256 distinct values: the separate value array)."""
    rng = np.random.default_rng([seed, count, 0x5369676E])
    top = 100 if mode == "palette" else 1000
    x = rng.integers(1, top + 1, size=count, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=count)
    if mode == "array":
        assert count >= 2003
        x[:1000] = np.arange(1, 1001)
        x[1000:2000] = -np.arange(1, 1001)
        x[2000:2003] = (INT32_MIN, INT32_MAX, -1)
        x = x[rng.permutation(count)]
    elif mode != "palette":
        raise ValueError(mode)
    return x


def with_signed_values(A, mode, seed=0):
    """The fused_ref matrix A with its values replaced by signed ones."""
    return F.Coo(A.nrows, A.ncols, A.i, A.j, signed_values(A.nnz, mode, seed))


def bit_patterns(x):
    """int32 values -> the u32 words the signed loader stores."""
    x = np.asarray(x, dtype=np.int64)
    assert x.min(initial=0) >= INT32_MIN and x.max(initial=0) <= INT32_MAX
    return (x & 0xFFFFFFFF).astype(np.uint32)


def residues(A, p, transpose=False):
    """exact_ref.Coo of A (or A^T) with values a % p as Python ints (Python's % is the true residue)."""
    i, j = (A.j, A.i) if transpose else (A.i, A.j)
    nr, nc = (A.ncols, A.nrows) if transpose else (A.nrows, A.ncols)
    M = X.Coo(nr, nc, i, j, np.zeros(A.nnz, dtype=np.int64))
    M.x = np.array([int(a) % p for a in A.x], dtype=object)
    return M


def write_mtx(path, nrows, ncols, i, j, x):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n%signed entries\n")
        f.write(f"{nrows} {ncols} {len(i)}\n")
        f.write("".join(f"{int(a) + 1} {int(b) + 1} {int(c)}\n" for a, b, c in zip(i, j, x)))
    return str(path)


def write_block(path, rows, cols, words, banner="%%MatrixMarket matrix array integer general\n"):
    """`words` row-major (rows x cols) -> a column-major array file."""
    w = np.array([int(q) for q in words], dtype=object).reshape(rows, cols)
    with open(path, "w") as f:
        f.write(banner + f"{rows} {cols}\n" + "".join(f"{int(w[r, c])}\n" for c in range(cols) for r in range(rows)))
    return str(path)


def read_block(path):
    """(rows, cols, row-major list of Python ints) of an array file."""
    with open(path) as f:
        lines = [ln for ln in f if not ln.startswith("%")]
    rows, cols = (int(t) for t in lines[0].split())
    w = [int(t) for t in lines[1:1 + rows * cols]]
    return rows, cols, [w[c * rows + r] for r in range(rows) for c in range(cols)]


def incidence(vertices, edges, seed=0):
    """The edge x vertex incidence matrix of a connected graph: a spanning path through a random order of the vertices,
    then random further edges; row e has +1 at one end and -1 at the other.  Its right kernel over any field is the
    constants (the graph is connected), as long as the entries mean +1 and -1."""
    assert edges >= vertices - 1
    rng = np.random.default_rng([seed, vertices, edges])
    order = rng.permutation(vertices)
    ends = [(int(order[k]), int(order[k + 1])) for k in range(vertices - 1)]
    while len(ends) < edges:
        a, b = (int(t) for t in rng.integers(0, vertices, size=2))
        if a != b:
            ends.append((a, b))
    ends = [ends[k] for k in rng.permutation(edges)]
    i = np.repeat(np.arange(edges, dtype=np.int64), 2)
    j = np.array([v for e in ends for v in e], dtype=np.int64)
    x = np.tile(np.array([1, -1], dtype=np.int64), edges)
    return F.Coo(edges, vertices, i, j, x)


def signed_sums(A, transpose=False):
    """The signed integer row sums of A (column sums with transpose), exact in float64 -- asserted."""
    assert int(np.abs(A.x).sum()) < 1 << 53
    idx, size = (A.j, A.ncols) if transpose else (A.i, A.nrows)
    return np.bincount(idx, weights=A.x.astype(np.float64), minlength=size).astype(np.int64)


def scaled_rows(s, o, p):
    """Reference (b): the block whose row r is ((s_r mod p) * o_k mod p)_k, flat u64; s signed int64 integers.
    Where o_k = p - a_k with a small a_k (the "ramp" and "max" operands) and |a_k s_r| < 2^62 the word is
    (-(a_k s_r)) mod p in int64 (numpy's % with a positive modulus is the non-negative residue); every other word is
    computed in Python integers."""
    s = np.asarray(s, dtype=np.int64)
    a = [p - int(ok) for ok in o]
    out = np.zeros((len(s), len(o)), dtype=np.uint64)
    if p < 1 << 62 and all(0 < ak < 1 << 4 for ak in a):
        small = np.abs(s) < 1 << 58
        for k, ak in enumerate(a):
            out[small, k] = ((-(s[small] * ak)) % np.int64(p)).astype(np.uint64)
        rest = np.flatnonzero(~small)
    else:
        rest = np.arange(len(s))
    if rest.size:
        uniq, inv = np.unique(s[rest], return_inverse=True)
        table = np.array([[(int(u) % p) * int(ok) % p for ok in o] for u in uniq], dtype=np.uint64).reshape(-1, len(o))
        out[rest] = table[inv.reshape(-1)]
    return out.reshape(-1)


def apply_ints(A, x, p, transpose=False):
    """A x (or A^T x) mod p for one vector of Python ints, entry by entry in Python ints."""
    out = [0] * (A.ncols if transpose else A.nrows)
    r, c = (A.j, A.i) if transpose else (A.i, A.j)
    for a, b, v in zip(r, c, A.x):
        out[int(a)] += int(v) * int(x[int(b)])
    return [w % p for w in out]
