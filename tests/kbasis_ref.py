"""Plain-Python restatement of the kernel basis (include/blz.h: blz_block_rref, blz_kernel_basis) and generators of
blocks and matrices with a known answer.  Not a test module: test_kernel_basis_host.py and test_gpu_kernel_basis.py
import it.  Arithmetic on Python ints (object arrays), so every prime below 2^62 is exact."""
import numpy as np


def _obj(a):
    return np.array([[int(w) for w in row] for row in a], dtype=object).reshape(len(a), -1)


def rref(block, p, n):
    """Canonical RREF of the row space of `block` (rows x n) mod p: (E as n x n object array, rank, pivot columns)."""
    A = _obj(block) % p if len(block) else np.zeros((0, n), dtype=object)
    r, piv = 0, []
    for c in range(n):
        if r == A.shape[0]:
            break
        nz = np.nonzero(A[r:, c] != 0)[0]
        if len(nz) == 0:
            continue
        i = r + int(nz[0])
        A[[r, i]] = A[[i, r]]
        A[r] = A[r] * pow(int(A[r, c]), p - 2, p) % p
        f = A[:, c].copy()
        f[r] = 0
        A = (A - np.outer(f, A[r])) % p
        piv.append(c)
        r += 1
    E = np.zeros((n, n), dtype=object)
    E[:r] = A[:r]
    return E, r, piv


def null_basis(E, s, piv, n, p):
    """Z0 (n x n, columns beyond n - s zero): the canonical null basis of the RREF E (rank s, pivots piv)."""
    Z = np.zeros((n, n), dtype=object)
    if s == 0:
        for f in range(n):
            Z[f, f] = 1
        return Z
    free = [f for f in range(n) if f not in piv]
    for jj, f in enumerate(free):
        Z[f, jj] = 1
        for i in range(s):
            Z[piv[i], jj] = (-int(E[i, f])) % p
    return Z


def kernel_basis(V, T, p, n):
    """Steps 1-4 of blz_kernel_basis: dict(k, s, basis (rows x k), z (n x n), Y)."""
    E1, s, P = rref(T, p, n)
    Z0 = null_basis(E1, s, P, n, p)
    Vo = _obj(V)
    Y = Vo.dot(Z0) % p if s > 0 else Vo % p
    E2, k, Q = rref(Y, p, n)
    z = np.zeros((n, n), dtype=object)
    for j, q in enumerate(Q):
        z[:, j] = Z0[:, q]
    return dict(k=k, s=s, basis=Y[:, Q] if k else np.zeros((Y.shape[0], 0), dtype=object), z=z, Y=Y)


def random_rref(rng, r, n, p):
    """A random RREF of rank r (n x n, rows r..n-1 zero) and its pivot columns."""
    piv = sorted(rng.choice(n, size=r, replace=False).tolist())
    B = np.zeros((n, n), dtype=object)
    for i, c in enumerate(piv):
        B[i, c] = 1
        for f in range(c + 1, n):
            if f not in piv:
                B[i, f] = int(rng.integers(0, p))
    return B, piv


def planted_block(rng, R, B, r, p, last_row=False):
    """V = U B (R x n uint64, RREF(V) = B exactly): U has entries in {0, 1}, at most two ones per row, and an r x r
    identity at random rows.  last_row: row r-1 of B appears in the final row only (an early exit that skips rows misses
    the last pivot)."""
    n = B.shape[1]
    Bu = np.array([[int(w) for w in row] for row in B[:max(r, 1)]], dtype=np.uint64)
    V = np.zeros((R, n), dtype=np.uint64)
    if r == 0:
        return V
    pool = r - 1 if last_row else r
    P = np.uint64(p)
    for _ in range(2):
        if pool == 0:
            break
        pick = rng.integers(0, pool, size=R)
        on = rng.integers(0, 2, size=R).astype(bool)
        add = Bu[pick]
        add[~on] = 0
        V = (V + add) % P
    rows = rng.choice(R - 1 if last_row else R, size=r, replace=False)
    for j in range(r):
        V[rows[j]] = Bu[j]
    if last_row:
        V[rows[r - 1]] = Bu[0] if r > 1 else 0
        V[R - 1] = Bu[r - 1]
    return V


def write_array(path, cols):
    """MatrixMarket "array integer general", column-major (what blz_save_block writes)."""
    cols = [list(map(int, c)) for c in cols]
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix array integer general\n")
        f.write("%block of kernel vectors\n")
        f.write(f"{len(cols[0]) if cols else 0} {len(cols)}\n")
        for c in cols:
            for w in c:
                f.write(f"{w}\n")


def planted_kernel_matrix(path, nrows, ncols, deps, seed, right=False, per_row=6, relations=None):
    """A sparse MatrixMarket matrix whose left (right) kernel has dimension `deps` over any large prime: random sparse
    rows (columns), then `deps` of them replaced by the sum of two others (appended to `relations` as (t, a, b):
    e_t - e_a - e_b is a kernel vector)."""
    rng = np.random.default_rng(seed)
    lines = nrows if not right else ncols
    width = ncols if not right else nrows
    vecs = []
    for _ in range(lines):
        idx = rng.choice(width, size=per_row, replace=False)
        vecs.append({int(c): int(rng.integers(1, 4)) for c in idx})
    targets = rng.choice(lines, size=deps, replace=False)
    others = [i for i in range(lines) if i not in set(targets.tolist())]
    for t in targets:
        a, b = rng.choice(others, size=2, replace=False)
        v = dict(vecs[a])
        for c, x in vecs[b].items():
            v[c] = v.get(c, 0) + x
        vecs[t] = v
        if relations is not None:
            relations.append((int(t), int(a), int(b)))
    ent = []
    for i, v in enumerate(vecs):
        for c, x in sorted(v.items()):
            ent.append((i, c, x) if not right else (c, i, x))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n")
        f.write(f"{nrows} {ncols} {len(ent)}\n")
        for i, j, x in ent:
            f.write(f"{i + 1} {j + 1} {x}\n")
    return path
