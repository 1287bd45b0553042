"""Helpers of the wide value mode's tests: matrices whose entries are any residue below p, their limbs and files, and
expectations in plain Python integers.  Nothing here calls the library.

A wide entry is a canonical residue a, 0 <= a < p < 2^62, handed to the library as two u32 limbs (a = lo + 2^32 hi).
Two references:
  (a) exact_ref's spmv / trajectory fed a Coo of the residues (int64 holds them);
  (b) a closed form: when every block row of the operand is the same row o, y[r, k] = (s_r mod p) * o_k mod p with s_r the
      integer sum of row r's residues (three 21-bit limbs summed by np.bincount, exact below 2^53 -- asserted).
"""
import numpy as np

import exact_ref as X
import fused_ref as F
from signed_ref import apply_ints, read_block, write_block, write_mtx   # noqa: F401  (shared with the signed mode's tests)

LIMB = 21


def specials(p):
    """The extreme operands of the rule acc += lo * x + hi * x': both sides of 2^32, the top of the field, a value with
    lo = 0 and one with lo = 0xFFFFFFFF at the largest high limb that has it, and 0 and 1.  Distinct residues, sorted."""
    hmax = (p - 1) >> 32
    top_ff = (hmax << 32) | 0xFFFFFFFF
    if top_ff >= p:
        top_ff = (max(hmax - 1, 0) << 32) | 0xFFFFFFFF
    vals = {0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, p - 1, p - (1 << 32), hmax << 32, top_ff}
    return sorted({v % p for v in vals})       # (below 2^32 the same list, reduced: such a prime has no wide residue)


def wide_values(count, mode, p, seed=0):
    """palette: at most 256 distinct residues, the specials among them; array: more than 256 distinct residues uniform in
    [0, p) plus the specials; allmax: every entry p - 1 (both limbs at their largest in every slot)."""
    rng = np.random.default_rng([seed, count, 0x57494445])
    sp = np.array(specials(p), dtype=np.int64)
    if mode == "allmax":
        return np.full(count, p - 1, dtype=np.int64)
    if mode == "palette":
        pool = np.unique(np.concatenate([sp, rng.integers(0, p, size=180, dtype=np.int64)]))
        assert len(pool) <= 256
        x = pool[rng.integers(0, len(pool), size=count)]
        k = min(count, len(sp))
        x[:k] = sp[:k]
        return x[rng.permutation(count)]
    if mode == "array":
        x = rng.integers(0, p, size=count, dtype=np.int64)
        assert count >= 300 + len(sp)
        x[:len(sp)] = sp
        x = x[rng.permutation(count)]
        assert len(np.unique(x)) > 256
        return x
    raise ValueError(mode)


def with_wide_values(A, mode, p, seed=0):
    """The fused_ref matrix A with its values replaced by residues below p."""
    return F.Coo(A.nrows, A.ncols, A.i, A.j, wide_values(A.nnz, mode, p, seed))


def limbs(x):
    """residues -> (low limbs, high limbs) as u32 arrays"""
    x = np.asarray(x, dtype=np.int64)
    assert x.min(initial=0) >= 0
    return (x & 0xFFFFFFFF).astype(np.uint32), (x >> 32).astype(np.uint32)


def residues(A, transpose=False):
    """exact_ref.Coo of A (or A^T): its values already are the residues."""
    i, j = (A.j, A.i) if transpose else (A.i, A.j)
    nr, nc = (A.ncols, A.nrows) if transpose else (A.nrows, A.ncols)
    return X.Coo(nr, nc, i, j, A.x)


def int_sums(idx, vals, size):
    """sum of the non-negative integers vals (below 2^63) per index, as an object array of Python integers"""
    vals = np.asarray(vals, dtype=np.int64)
    assert vals.min(initial=0) >= 0 and len(vals) < 1 << (53 - LIMB)
    out = np.zeros(size, dtype=object)
    for q in range(3):
        part = ((vals >> (LIMB * q)) & ((1 << LIMB) - 1)).astype(np.float64)
        out = out + (np.bincount(idx, weights=part, minlength=size).astype(np.int64).astype(object) << (LIMB * q))
    return out


def to_u64(obj):
    return np.array([int(t) for t in obj], dtype=np.uint64)


def mul_small_mod(s, a, p):
    """(a * s) mod p for a u64 array of residues s and a small integer a, by doubling in u64 (p < 2^62: no wrap)"""
    s = np.asarray(s, dtype=np.uint64)
    P = np.uint64(p)
    acc = np.zeros_like(s)
    for bit in bin(a)[2:]:
        acc = acc + acc
        acc = np.where(acc >= P, acc - P, acc)
        if bit == "1":
            acc = acc + s
            acc = np.where(acc >= P, acc - P, acc)
    return acc


def scaled_rows(s, o, p):
    """Reference (b): the block whose row r is (s_r * o_k mod p)_k, flat u64; s a u64 array of residues.
    o_k = p - a_k with a small a_k (the "ramp" and "max" operands): the word is -(a_k s_r) mod p; else Python integers."""
    s = np.asarray(s, dtype=np.uint64)
    out = np.zeros((len(s), len(o)), dtype=np.uint64)
    for k, ok in enumerate(o):
        a = p - int(ok)
        if 0 < a < 1 << 8:
            t = mul_small_mod(s, a, p)
            out[:, k] = np.where(t == 0, np.uint64(0), np.uint64(p) - t)
        else:
            out[:, k] = to_u64((s.astype(object) * int(ok)) % p)
    return out.reshape(-1)


def row_residues(A, p, transpose=False):
    """(s_r mod p) of the rows of A (columns with transpose), u64"""
    idx, size = (A.j, A.ncols) if transpose else (A.i, A.nrows)
    return to_u64(int_sums(idx, A.x, size) % p)


def iteration_expectation(A, n, p, o):
    """Reference (b) for one iteration from v = rows of o, A = M of a left kernel: tmp[t, k] = w_t o_k with w = A^T 1,
    Av[c, k] = s_c o_k with s = A w, vtAv[i][j] = o_i o_j sum_c s_c, vtAAv[i][j] = o_i o_j sum_c s_c^2, all mod p (w and s
    are taken mod p on the way: the products are of residues)."""
    w = row_residues(A, p, transpose=True)
    terms = (A.x.astype(object) * w.astype(object)[A.j]) % p
    s = to_u64(int_sums(A.i, np.array([int(t) for t in terms], dtype=np.int64), A.nrows) % p)
    so = s.astype(object)
    t1, t2 = int(so.sum()) % p, int((so * so).sum()) % p
    return dict(v=np.tile(np.array(o, dtype=np.uint64), A.nrows), tmp=scaled_rows(w, o, p), Av=scaled_rows(s, o, p),
                vtAv=np.array([o[i] * o[j] * t1 % p for i in range(n) for j in range(n)], dtype=np.uint64),
                vtAAv=np.array([o[i] * o[j] * t2 % p for i in range(n) for j in range(n)], dtype=np.uint64))
