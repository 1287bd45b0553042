"""The integer scheme of the device block algebra's matrix-core recombination (csrc/blz_devmfma.hip, k_dm_prep and
k_dm_combine; the layout and the start are csrc/blz_devmfma_plan.h's) restated in plain Python integers, in the manner of
mfma_digits_ref.model_update: Z = sum_t X_t A_t at p = 2^61 - 1 for n = 8 or 16 and 1..4 terms, K' = 8 n nterms.

Nothing here calls the library.  The inner products of that file keep k_block_dot_mfma's scheme and its fold interval (64
tiles of 64 rows, accumulators from 2^30): mfma_digits_ref.model_dot and test_mfma_digits_ref.py are their model.

    START, SUM_MAX, FCONST     the accumulator start derived for the longest K', the largest digit sum, the correction
    model_combine              the kernels' arithmetic step by step, with the range the int32 accumulators take
    combine_exact              plain integer arithmetic
    tiled                      one period of rows repeated down to `rows` rows (the update is row-local)
"""
import operator

import numpy as np

import mfma_digits_ref as R

P = R.P
MAX_TERMS = 4
KMAX = 8 * 16 * MAX_TERMS                   # DM_KMAX
# S = START + sum over K' of u d, u a byte in [0, 255], d a signed digit in [-128, 127]: the least start that keeps
# S >= 0 at the longest K' (DM_START)
START = KMAX * 255 * 128
SUM_MAX = START + KMAX * 255 * 127          # DM_SUM_MAX
FCONST = (-sum(START << (8 * t) for t in range(8))) % P


def kprime(n, nterms):
    return 8 * n * nterms


def lo_end(n, nterms):
    return START - kprime(n, nterms) * 255 * 128


def hi_end(n, nterms):
    return START + kprime(n, nterms) * 255 * 127


def images(a0, a1, n):
    """[set][tile column][K' word] -> coefficient, as dm_coef lays them out.  a0 / a1: lists of n x n coefficient lists
    (flat), None for a zero panel; a1 = None is the single form.  n = 16: one image per output; n = 8: ONE image, Z0 in tile
    columns 0..7 and Z1 (or zeros) in 8..15."""
    nterms = len(a0)
    pair = a1 is not None

    def at(a, t, k, c):
        return 0 if a is None or a[t] is None else int(a[t][k * n + c])

    if n == 16:
        sets = [a0, a1] if pair else [a0]
        return [[[at(a, kk // 16, kk % 16, col) for kk in range(16 * nterms)] for col in range(16)] for a in sets]
    return [[[at(a0 if col < 8 else (a1 if pair else None), kk // 8, kk % 8, col & 7) for kk in range(8 * nterms)]
             for col in range(16)]]


def model_combine(xs, a0, a1, rows, n, cols=None):
    """(z0, z1, lo, hi, s_lo, s_hi): Z0 = sum_t xs[t] a0[t] and, with a1 not None, Z1 the same with a1 (else z1 is None),
    as k_dm_prep and k_dm_combine compute them; blocks are flat lists of rows * n words.  lo / hi: the least and largest
    value an int32 accumulator holds, from its start through every MFMA of 64 products; s_lo / s_hi: the same over the
    finished digit sums alone.  cols: the tile columns to compute (all 16 by default; the others come out as None)."""
    assert n in (8, 16) and 1 <= len(xs) <= MAX_TERMS and len(a0) == len(xs) and (a1 is None or len(a1) == len(xs))
    nterms, pair = len(xs), a1 is not None
    cols = range(16) if cols is None else cols
    img = []
    for coef in images(a0, a1, n):
        Bt = {(t, col): [R.signed_digit(R.rot61(coef[col][kp >> 3], 8 * (kp & 7)), t) for kp in range(kprime(n, nterms))]
              for t in range(8) for col in cols}
        start = {key: 128 * sum(b) + START for key, b in Bt.items()}
        img.append((Bt, start))
    lo = hi = s_lo = s_hi = START
    z0, z1 = [], []
    for r in range(rows):
        A = [R.s8(b) for x in xs for w in x[r * n:(r + 1) * n] for b in R.word_bytes(int(w))]
        tile = []
        for Bt, start in img:
            row = [None] * 16
            for col in cols:
                total = 0
                for t in range(8):
                    acc = start[t, col]
                    lo, hi = min(lo, acc), max(hi, acc)
                    b = Bt[t, col]
                    for k0 in range(0, len(A), 64):                 # one MFMA: 64 products
                        acc += sum(map(operator.mul, A[k0:k0 + 64], b[k0:k0 + 64]))
                        lo, hi = min(lo, acc), max(hi, acc)
                    assert -(1 << 31) <= lo and hi < 1 << 31
                    s_lo, s_hi = min(s_lo, acc), max(s_hi, acc)
                    total += (acc & 0xFFFFFFFF) << (8 * t)          # the kernel reads the accumulator as u32
                row[col] = (total + FCONST) % P
            tile.append(row)
        if n == 16:
            z0 += tile[0]
            if pair:
                z1 += tile[1]
        else:
            z0 += tile[0][:8]
            if pair:
                z1 += tile[0][8:]
    return z0, (z1 if pair else None), lo, hi, s_lo, s_hi


def combine_exact(xs, a, rows, n):
    """sum_t xs[t] a[t] mod p in plain integers (a[t] None: a zero panel); flat list of rows * n words"""
    out = []
    for r in range(rows):
        for j in range(n):
            out.append(sum(int(x[r * n + k]) * int(at[k * n + j]) for x, at in zip(xs, a) if at is not None for k in range(n)) % P)
    return out


def tiled(period_words, rows, n):
    """one period (flat list, a whole number of rows) repeated down to `rows` rows: uint64 array of shape (rows, n)"""
    one = np.array(period_words, dtype=np.uint64).reshape(-1, n)
    return np.tile(one, (rows // one.shape[0] + 1, 1))[:rows]
