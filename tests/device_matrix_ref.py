"""Case list and numpy reference of the device matrix build (blz_set_matrix_device, csrc/blz_devmat.hip).

The reference product is exact: Python integers in numpy `object` arrays, reduced once at the end.  The case lists are shared
by tests/test_host_device_matrix.py (which shows that they reach every template instantiation of the kernels and that the
reference agrees with the CPU oracle) and tests/test_gpu_device_matrix.py (which runs them on the GPU).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# csrc/blz_devmat.h: counters per workgroup of the scan, tile sums per round of the one workgroup that scans them
SCAN_TILE, SCAN_CHUNK = 1024, 256
PAL_MAX = 256

P16, P31, P32, P61, P61B = 65537, (1 << 31) - 1, (1 << 32) - 5, (1 << 61) - 1, (1 << 61) - 31
PRIMES = (P16, P31, P32, P61, P61B)
GOLDENS = ("quirks40x30", "rand300x200", "graph200x600", "trefethen20", "rand3000x2000")
WIDTHS = (1, 5, 8, 16)


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


# (matrix, p, n, idx_bytes, val_bytes): every golden matrix, every prime, every width, both index widths and both value
# widths at least once -- a covering subset of the product, not the product
ORACLE_CASES = tuple(
    (GOLDENS[k % 5], PRIMES[(k + k // 5) % 5], WIDTHS[k % 4], (4, 8)[(k // 2) % 2], (4, 8)[((k + 1) // 2) % 2])
    for k in range(10))


def scan_row_counts():
    """the row counts of the scan / scatter edge cases: the issue's list, and one below, at and above the point where the
    rows + 1 counters fill a tile (SCAN_TILE) and a round of tile sums (SCAN_TILE * SCAN_CHUNK)"""
    rows = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 1048577}
    for full in (SCAN_TILE, SCAN_TILE * SCAN_CHUNK):
        rows.update({full - 2, full - 1, full})         # rows + 1 = full - 1, full, full + 1 counters
    return sorted(rows)


def edge_triplets(rows, val_bytes, p=P16):
    """a rows x rows matrix with entries in the first row, the last row and on both sides of every tile boundary of the scan
    (of the row counters AND of the column counters: column = rows - 1 - row), nothing anywhere else; two entries per such
    row.  val_bytes 0: ones (x is None)."""
    marks = {0, rows - 1}
    for b in range(SCAN_TILE, rows + 2, SCAN_TILE):
        marks.update(r for r in (b - 2, b - 1, b, b + 1) if 0 <= r < rows)
    i = np.array(sorted(marks), dtype=np.int64)
    i = np.concatenate([i, i])
    j = np.concatenate([rows - 1 - i[:len(i) // 2], (i[len(i) // 2:] * 7 + 3) % rows])
    order = np.random.default_rng([rows, 11]).permutation(len(i))      # not sorted by row
    i, j = i[order], j[order]
    if val_bytes == 0:
        return i, j, None
    x = np.random.default_rng([rows, 5]).integers(1, p, size=len(i), dtype=np.uint64)
    x[0], x[-1] = p - 1, 1
    return i, j, x


# (rows, idx_bytes, val_bytes) of the edge cases: all three value forms and both index forms come round
EDGE_CASES = tuple((rows, (4, 8)[k % 2], (0, 4, 8)[k % 3]) for k, rows in enumerate(scan_row_counts()))


def instantiations_reached():
    """the (idx_bytes, val_bytes) pairs the two case lists launch"""
    return {(ib, vb) for _, _, _, ib, vb in ORACLE_CASES} | {(ib, vb) for _, ib, vb in EDGE_CASES}


def spmv_ref(nrows, ncols, i, j, x, X, transpose, n, p):
    """y = M X (transpose False) / M^T X mod p as flat u64 words; x None = ones; duplicates add up.  Exact integers."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    ri, ci = (j, i) if transpose else (i, j)
    rows_out = ncols if transpose else nrows
    y = np.zeros((rows_out, n), dtype=np.uint64)
    if len(i) == 0:
        return y.reshape(-1)
    X = np.asarray(X, dtype=np.uint64).reshape(-1, n)
    terms = X[ci].astype(object)
    if x is not None:
        terms = terms * np.asarray(x).astype(object)[:, None]
    touched, inv = np.unique(ri, return_inverse=True)
    acc = np.zeros((len(touched), n), dtype=object)
    np.add.at(acc, inv, terms)
    y[touched] = (acc % p).astype(np.uint64)
    return y.reshape(-1)


def residues(rows, n, p, seed):
    """random residues with 0 and p - 1 in every column"""
    rng = np.random.default_rng([seed, rows, n])
    w = rng.integers(0, p, size=(rows, n), dtype=np.uint64)
    if rows >= 2:
        for col in range(n):
            a, b = rng.choice(rows, 2, replace=False)
            w[a, col], w[b, col] = 0, p - 1
    return w
