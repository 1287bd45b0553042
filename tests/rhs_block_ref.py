"""Solves with k right-hand sides restated in plain Python integers: the operator with k border columns / rows written out.

M X = B (right) is the search for kernel vectors of M' = [M | B] whose last k coordinates are -e_i; X M = B (left) the same
for M' = [M ; B].  The library keeps B out of the matrix and applies it as a dense border behind each product, for all k
columns in one pass; here M' is simply built, the way rhs_ref.augmented builds it for one b, and handed to exact_ref's
spmv / iteration / trajectory.

    augmented        the triplets of M' (the k border columns / rows last; zero entries of B left out)
    planted          k seeded x0_i and B with column i = M x0_i resp. x0_i M
    columns / rows   between the list of k vectors and the len x k row-major block the library takes
    write_block      B as the "array integer general" file the command line reads (column-major)
    basis_border     the border part W (k x kb) of the kernel vectors in the span of a final block's columns
    solvable         for each i: is e_i in W's column space (system i is solved from this basis)
    verdict          the restatement run to its stop: iterations, hash of the final block, which systems it solves
    recorded         the verdict of the one case too long to restate in every test run (rand3000x2000: most of a minute
                     of Python integers), kept in tests/golden/rhs_block_rand3000x2000.json; `python rhs_block_ref.py`
                     recomputes and rewrites it
"""
import json
import os

import numpy as np

import exact_ref as X
import rhs_ref as R


def augmented(M, cols, right):
    """exact_ref.Coo of [M | b_0 ... b_{k-1}] (right) or of M with the rows b_i appended; cols = the k vectors."""
    k = len(cols)
    ii, jj, xx = list(M.i), list(M.j), list(M.x)
    for c, b in enumerate(cols):
        assert len(b) == (M.nrows if right else M.ncols)
        for r, w in enumerate(b):
            if int(w):
                ii.append(r if right else M.nrows + c)
                jj.append(M.ncols + c if right else r)
                xx.append(int(w))
    return X.Coo(M.nrows + (0 if right else k), M.ncols + (k if right else 0), ii, jj, xx)


def planted(M, right, p, k, seed):
    """(x0s, cols): k planted solutions and their right-hand sides, system i seeded with seed + i."""
    pairs = [R.planted(M, right, p, seed + i) for i in range(k)]
    return [x for x, _ in pairs], [b for _, b in pairs]


def rows(cols):
    """the k vectors as the len x k block (numpy u64, row-major) of blz_set_matrix_rhs_block"""
    return np.array([[int(w) for w in col] for col in cols], dtype=np.uint64).T.copy()


def columns(block):
    """the k columns of a len x k block as lists of Python integers"""
    return [[int(w) for w in block[:, i]] for i in range(block.shape[1])]


def write_block(path, cols, p, signed=True):
    """column-major, every third word as its negative representative: true residues"""
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix array integer general\n" + f"{len(cols[0])} {len(cols)}\n")
        for col in cols:
            f.write("".join(f"{w - p if signed and q % 3 == 0 else w}\n" for q, w in enumerate(col)))
    return str(path)


def _rref(A, ncols, p):
    """row-reduces the list of rows A over its first ncols columns in place; returns the pivot columns"""
    piv, r = [], 0
    for c in range(ncols):
        q = next((t for t in range(r, len(A)) if A[t][c]), None)
        if q is None:
            continue
        A[r], A[q] = A[q], A[r]
        inv = pow(A[r][c], -1, p)
        A[r] = [w * inv % p for w in A[r]]
        for t in range(len(A)):
            if t != r and A[t][c]:
                f = A[t][c]
                A[t] = [(a - f * b) % p for a, b in zip(A[t], A[r])]
        piv.append(c)
        r += 1
    return piv


def basis_border(A, v, n, k, p, right):
    """W: the last k rows of Y = v Z, Z = a basis of the combinations of v's columns that M' sends to zero (what
    blz_kernel_basis keeps, up to a change of basis, which does not change W's column space)."""
    T = np.array(X.spmv(A, v, not right, n, p), dtype=object).reshape(-1, n)
    rows_t = [[int(w) for w in row] for row in T if any(row)]
    piv = _rref(rows_t, n, p) if rows_t else []
    free = [c for c in range(n) if c not in piv]
    Z = []                                       # one combination (length n) per free column
    for f in free:
        z = [0] * n
        z[f] = 1
        for t, c in enumerate(piv):
            z[c] = (-rows_t[t][f]) % p
        Z.append(z)
    V = np.array([int(w) for w in v], dtype=object).reshape(-1, n)[-k:]
    return [[sum(int(V[i][c]) * z[c] for c in range(n)) % p for z in Z] for i in range(k)]


def solvable(W, p):
    """[e_i in the column space of W for i < k]: reduce [W | I] over W's columns; e_i is in the span exactly when its
    reduced column is zero below the rank."""
    k = len(W)
    kb = len(W[0]) if W else 0
    A = [list(W[i]) + [int(i == j) for j in range(k)] for i in range(k)]
    r = len(_rref(A, kb, p))
    return [not any(A[t][kb + i] for t in range(r, k)) for i in range(k)]


def rank(W, p):
    A = [list(row) for row in W]
    return len(_rref(A, len(A[0]), p)) if A and A[0] else 0


def init_v(M, right, n, p, k):
    return X.init_v((M.ncols if right else M.nrows) + k, n, p)


def verdict(M, cols, right, n, p):
    """The restatement run to its stop on [M | cols] / [M ; cols]: what a solve of these systems must find."""
    k = len(cols)
    A = augmented(M, cols, right)
    _, end = X.trajectory(A, n, p, right)
    W = basis_border(A, end["v"], n, k, p, right)
    return {"iterations": end["iterations"], "v_sha": X.sha(end["v"]), "w_rank": rank(W, p),
            "solvable": [int(s) for s in solvable(W, p)]}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDED_CASE = {"name": "rand3000x2000", "right": True, "p": X.P61, "n": 16, "k": 5, "seed": 55}
RECORDED_PATH = os.path.join(GOLDEN, "rhs_block_rand3000x2000.json")


def recorded():
    with open(RECORDED_PATH) as f:
        rec = json.load(f)
    assert rec["case"] == RECORDED_CASE, "the recorded case is not the one asked for: run rhs_block_ref.py"
    return rec["verdict"]


if __name__ == "__main__":
    c = RECORDED_CASE
    M = X.load_mtx(os.path.join(GOLDEN, c["name"] + ".mtx"), c["p"])
    out = {"case": c, "verdict": verdict(M, planted(M, c["right"], c["p"], c["k"], c["seed"])[1], c["right"], c["n"], c["p"])}
    with open(RECORDED_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)
