"""Case lists and numpy restatement of the device renumbering (blz_set_matrix_device_ordered, csrc/blz_devorder.hip).

The order is blz_reorder's: rows sorted stably by their smallest column (rows without entries take the key ncols), then columns
sorted stably by their smallest NEW row.  Here it is `np.minimum.at` and a stable argsort: a minimum and a stable sort have one
answer, so the comparison with the host's blz.reorder and with the GPU is equality of integers.  The case lists are shared by
tests/test_host_device_order.py (which shows that the restatement is blz.reorder, and that the lists reach both index widths and
every pass count of the sort) and tests/test_gpu_device_order.py (which runs them on the GPU).
"""
import numpy as np

import device_matrix_ref as dm

# csrc/blz_devorder.h: items per workgroup of the sort, bits per digit pass
SORT_TILE, DIGIT_BITS = 256, 8

P16, P31, P32, P61 = dm.P16, dm.P31, dm.P32, dm.P61
PRIMES = (P16, P31, P32, P61)
GOLDENS = dm.GOLDENS
path = dm.path


def sort_passes(nkeys):
    """digit passes of a sort of keys in [0, nkeys]"""
    return -(-int(nkeys).bit_length() // DIGIT_BITS)


def stable_positions(key):
    """perm[item] = position of the item in a stable sort by key"""
    perm = np.empty(len(key), dtype=np.int32)
    perm[np.argsort(key, kind="stable")] = np.arange(len(key), dtype=np.int32)
    return perm


def order_ref(nrows, ncols, i, j):
    """(row_perm, col_perm) of blz_reorder as int32 arrays"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    key = np.full(nrows, ncols, dtype=np.int64)
    np.minimum.at(key, i, j)
    row_perm = stable_positions(key)
    key = np.full(ncols, nrows, dtype=np.int64)
    np.minimum.at(key, j, row_perm[i].astype(np.int64))
    return row_perm, stable_positions(key)


def numbering_ref(nrows, ncols, i, j, right):
    """(numbering of V's side, of TMP's side): rows of M live on V's side for a left kernel, on TMP's for a right one; a
    matrix without entries keeps the identity"""
    if len(i) == 0:
        rp, cp = np.arange(nrows, dtype=np.int32), np.arange(ncols, dtype=np.int32)
    else:
        rp, cp = order_ref(nrows, ncols, i, j)
    return (cp, rp) if right else (rp, cp)


# (matrix, p, n, right, idx_bytes, val_bytes): the golden files left and right, both index widths, values none / u32 / u64, the
# four primes -- a covering subset of the product
GOLDEN_CASES = tuple(
    (GOLDENS[k % 5], PRIMES[(k + k // 5) % 4], (1, 4, 8, 16)[k % 4], bool((k + k // 5) % 2), (4, 8)[(k // 2) % 2],
     (0, 4, 8)[k % 3])
    for k in range(12))

# (matrix, right, p, n) of the whole solves
SOLVE_CASES = tuple((name, right, p, n) for name in ("rand300x200", "quirks40x30") for right in (False, True)
                    for p, n in ((P16, 4), (P61, 8)))

SORT_ROWS = tuple(SORT_TILE * a + b for a, b in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (5, 3)))
SORT_COLS = (200, 300, 70000)          # keys in [0, ncols]: 1, 2 and 3 digit passes


def sort_cases():
    """(rows, cols, idx_bytes, val_bytes) of the sort's edge cases: every row count against every key range, and the point
    where the key of a row WITHOUT entries (ncols itself) needs one digit more than every column index does"""
    cases = [(rows, cols, (4, 8)[(a + b) % 2], (0, 4, 8)[(a + 2 * b) % 3])
             for a, rows in enumerate(SORT_ROWS) for b, cols in enumerate(SORT_COLS)]
    cases.append((SORT_TILE + 1, (1 << DIGIT_BITS) - 1, 4, 4))
    cases.append((SORT_TILE + 1, 1 << DIGIT_BITS, 8, 0))
    return tuple(cases)


def sort_triplets(rows, cols, val_bytes, p=P16):
    """a rows x cols matrix for the sort: every row on both sides of every tile boundary has entries, about one row in seven
    has none (in the middle, and the last two unless a tile boundary sits there), the smallest columns are drawn from a pool of about rows / 3 values between 0
    and cols - 1 -- so most keys are shared by several rows, and a sort that is not stable shows -- and the triplets are not
    sorted by row.  val_bytes 0: ones (x is None)."""
    rng = np.random.default_rng([rows, cols, 17])
    pool = np.unique(np.concatenate([rng.integers(0, cols, max(rows // 3, 2)), [0, cols - 1]]))
    empty = rng.random(rows) < 1 / 7
    empty[max(rows - 2, 0):] = True
    for b in range(SORT_TILE, rows, SORT_TILE):         # (a boundary between two rows that exist wins over the empty end)
        empty[b - 1:b + 1] = False
    empty[0] = False
    filled = np.flatnonzero(~empty)
    i = np.concatenate([filled, filled])
    least = rng.choice(pool, len(filled))
    j = np.concatenate([least, np.maximum(least, rng.integers(0, cols, len(filled)))])
    order = rng.permutation(len(i))
    i, j = i[order], j[order]
    if val_bytes == 0:
        return i, j, None
    x = rng.integers(1, p, size=len(i), dtype=np.uint64)
    x[0], x[-1] = p - 1, 1
    return i, j, x


def all_tied(rows, cols):
    """every row has its smallest entry in one column: the rows must stay in place"""
    r = np.arange(rows)
    return np.concatenate([r, r]), np.concatenate([np.full(rows, 3), 4 + (r * 5) % (cols - 4)])


def descending(rows):
    """row r has its only entry in column rows - 1 - r: all keys distinct and descending, the order is fully reversed"""
    r = np.arange(rows)
    return r, rows - 1 - r


def index_widths_reached():
    return {ib for *_, ib, _ in GOLDEN_CASES} | {ib for _, _, ib, _ in sort_cases()}


def pass_counts_reached():
    """pass counts of the row sort and of the column sort over the sort cases, and of the 4-pass case (30 x 2^24 + 5)"""
    return {sort_passes(cols) for _, cols, _, _ in sort_cases()} | {sort_passes(rows) for rows, _, _, _ in sort_cases()} \
        | {sort_passes(FOUR_PASS[1])}


FOUR_PASS = (30, (1 << 24) + 5)          # rows, columns: keys of the row sort in [0, 2^24 + 5] take four digits
