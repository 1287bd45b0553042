"""The matrix-core kernels' integer scheme (csrc/blz_dense_mfma.hip, csrc/ortho_img.h) restated in plain Python integers,
and inputs chosen by their BYTES, for p = 2^61-1 and block widths 8 and 16.

Nothing here calls the library or the oracle.  The vector-ALU kernels are bounded by a 128-bit sum and a reducer, and
all-(p-1) operands sit on that bound; these kernels contract base-256 digits in int32 accumulators, and their bounds are
digit bounds: the byte 0x00 (which XOR 0x80 turns into -128), the step between 0x7F and 0x80 (127 and -128), the carry
chain of the signed recoding of a coefficient, a rotation of a coefficient that wraps past bit 60, and -- in the inner
products -- the re-start of the accumulators after 64 tiles.  The bytes of p-1 are FE FF FF FF FF FF FF 1F: 126, 127 and
-97 after the XOR, near none of these.

    PATTERNS                       words below p named by their bytes
    const_block / cycle_block      blocks of them (numpy, built with full / tile: no loop over the rows)
    coef_const / coef_cycle / coef_rotation
                                   n x n coefficient matrices
    through_semi_inverse           VTAV and VTAAV that make semi_inverse + ortho_coeffs produce chosen c and vtAvd
    model_update / model_dot       the kernels' arithmetic step by step, with the range their accumulators take
    const_dot / cycle_dot / tiled_update
                                   closed forms the GPU tests compare with
"""
import collections
import operator

import numpy as np

import exact_ref as X

P = X.P61

_NAMES = ("zero", "one", "pm1", "bit60", "ff_x7", "top_7f", "top_80", "all_80", "all_7f", "alt_ff", "top_alt_00ff",
          "top_low7f", "low_80", "top_only", "low_ff")
PATTERNS = collections.namedtuple("Patterns", _NAMES)(
    0,                          # every byte 0x00 -> -128: drives an inner-product accumulator highest
    1,
    P - 1,                      # FE FF FF FF FF FF FF 1F, the vector-ALU kernels' bound
    1 << 60,
    0x00FFFFFFFFFFFFFF,         # seven bytes 0xFF -> 127 under a zero top byte
    0x1F7F7F7F7F7F7F7F,         # 0x7F -> -1 ...
    0x1F80808080808080,         # ... and 0x80 -> 0: the sign boundary of the left operand; +C carries in every byte
    0x0080808080808080,
    0x007F7F7F7F7F7F7F,
    0x00FF00FF00FF00FF,
    0x1F00FF00FF00FF00,
    0x1FFFFFFFFFFFFF7F,
    0x0000000000000080,         # one rotation by 8a lands on the top bits and wraps
    0x1F00000000000000,         # the top byte alone, at its largest: every rotation of it wraps (0x1000000000000000 is bit60)
    0x00000000000000FF,         # against ff_x7: every digit pair of s = 7 is (127, -128), the lowest an accumulator goes
)
L = len(PATTERNS)
assert all(0 <= w < P for w in PATTERNS)

# the constant pairs test_mfma_digits_ref.py finds (and asserts) as the worst of PATTERNS x PATTERNS
DOT_HIGHEST = ("zero", "zero")          # (-128)(-128) in all 8 digit pairs of s = 7: + 2^29 over the 2^30 start in 64 tiles
DOT_LOWEST = ("low_ff", "ff_x7")        # (127)(-128) in all 8 digit pairs of s = 7
UPDATE_HIGHEST = ("ff_x7", "all_7f")    # (block word, coefficient): digit sum S_t furthest above its 2^24 start
UPDATE_LOWEST = ("ff_x7", "all_80")     # ... and furthest below


def word(name):
    return getattr(PATTERNS, name)


# ------------------------------------------------------------------------------------------------ blocks


def const_block(w, rows, n):
    """rows x n, every word w (flat uint64)."""
    return np.full(rows * n, w, dtype=np.uint64)


def cycle_period(n, shift):
    """One period (L rows) of cycle_block as a list of rows of Python integers."""
    return [[PATTERNS[(r + k + shift) % L] for k in range(n)] for r in range(L)]


def cycle_block(rows, n, shift):
    """word (r, k) = PATTERNS[(r + k + shift) % L]: every column, every K' position of the update and every row position
    of an inner-product tile (L is odd, 16 and 64 are not multiples of it) sees every byte class."""
    one = np.array(cycle_period(n, shift), dtype=np.uint64)
    return np.tile(one, (rows // L + 1, 1))[:rows].reshape(-1)


# ------------------------------------------------------------------------------------------------ coefficients


def coef_const(w, n):
    return [w] * (n * n)


def coef_cycle(n, shift=0):
    return [PATTERNS[(k * n + j + shift) % L] for k in range(n) for j in range(n)]


def coef_rotation(n):
    """entry (k, j) = 2^((61 - 8 (k % 8)) % 61 + j % 8) mod p: rotated by 8a the multipliers land on 2^(j % 8) (a = k % 8:
    1, ..., 0x80, the digit the recoding turns into -128 with a carry), on the bits below the top, and on the wrap."""
    return [pow(2, (61 - 8 * (k % 8)) % 61 + j % 8, P) for k in range(n) for j in range(n)]


def through_semi_inverse(C, T, n, mixed):
    """(S, B, want_c, want_vd, want_d): with VTAV = S and VTAAV = B, semi_inverse gives the selector want_d and
    ortho_coeffs c = want_c and vtAvd = want_vd.  The update kernels read c and vtAvd from the panels the semi-inverse kernel
    writes, so a chosen coefficient has to come out of it.  S = -U with U the upper triangle of T (a zero on the diagonal
    becomes 1, so that U is invertible): then d is all ones, winv = -U^-1, vtAvd = -S = U and c = -winv B = U^-1 B, which
    is C for B = U C.  mixed: the odd rows of U are zero as well; the sweep selects the even columns (d alternates 1, 0),
    vtAvd keeps U's even columns, c's even columns are C's (even rows; the odd rows of c are zero with winv's), and c's odd
    columns come from vtAv: -winv S = U_ee^-1 U_eo, whatever words that gives."""
    keep = [k % 2 == 0 or not mixed for k in range(n)]
    U = [(T[k * n + j] if j > k else (T[k * n + k] or 1)) if j >= k and keep[k] else 0 for k in range(n) for j in range(n)]
    S = [(-u) % P for u in U]
    d = [int(keep[j]) for j in range(n)]
    Cm = [C[k * n + j] if keep[k] else 0 for k in range(n) for j in range(n)]
    B = [sum(U[k * n + m] * Cm[m * n + j] for m in range(n) if keep[m]) % P for k in range(n) for j in range(n)]
    want_vd = [U[k * n + j] if d[j] else 0 for k in range(n) for j in range(n)]
    return S, B, Cm, want_vd, d


# ------------------------------------------------------------------------------------------------ the digit scheme


def s8(u):
    """a byte XOR 0x80, read as a signed 8-bit integer: u - 128"""
    v = u ^ 0x80
    return v - 256 if v >= 128 else v


def rot61(x, sh):
    """x * 2^sh mod 2^61-1 as ortho_img.h computes it: a rotation of the 61-bit word"""
    assert 0 <= x < 1 << 61 and 0 <= sh < 61
    r = ((x << sh) & P) | (x >> (61 - sh))
    return x if sh == 0 else (0 if r == P else r)


def signed_digit(x, t):
    """digit t of x in signed base 256: byte t of x + 0x8080...80, minus 128"""
    y = x + 0x8080808080808080
    assert y < 1 << 64
    return ((y >> (8 * t)) & 0xFF) - 128


def word_bytes(w):
    return [(w >> (8 * a)) & 0xFF for a in range(8)]


ORTHO_START = 1 << 24
FCONST = (-sum(ORTHO_START << (8 * t) for t in range(8))) % P


def _chains(c, vd, winv, n):
    """coefficient of (chain, K' word kk, tile column) as ortho_img.h's coef_index lays them out: n = 16: [v | p] x [c ;
    vtAvd] and v x winv; n = 8: one chain, [v | p] x [[c | winv] ; [vtAvd | 0]]."""
    if n == 16:
        return [[[(c[kk * 16 + col] if kk < 16 else vd[(kk - 16) * 16 + col]) for col in range(16)] for kk in range(32)],
                [[winv[kk * 16 + col] for col in range(16)] for kk in range(16)]]
    one = []
    for kk in range(16):
        left = [(c[kk * 8 + col] if kk < 8 else vd[(kk - 8) * 8 + col]) for col in range(8)]
        right = [(winv[kk * 8 + col] if kk < 8 else 0) for col in range(8)]
        one.append(left + right)
    return [one]


def model_update(v, Av, pb, c, vd, winv, d, rows, n):
    """(v', p', lo, hi, s_lo, s_hi): the update as k_ortho_mfma_prep and k_ortho_mfma compute it.  lo / hi: the least and
    largest value an int32 accumulator holds, from its start through every step of 64 products; s_lo / s_hi: the same over
    the finished digit sums S_t alone."""
    assert n in (8, 16)
    chains = _chains(c, vd, winv, n)
    # B_t[K'][col] per chain and the accumulator starts
    img = []
    for ch in chains:
        Bt = [[[signed_digit(rot61(ch[kp >> 3][col], 8 * (kp & 7)), t) for kp in range(8 * len(ch))] for col in range(16)]
              for t in range(8)]
        start = [[128 * sum(Bt[t][col]) + ORTHO_START for col in range(16)] for t in range(8)]
        img.append((Bt, start))
    lo = hi = s_lo = s_hi = ORTHO_START
    out_v, out_p = [], []
    for r in range(rows):
        vr, ar, pr = (blk[r * n:(r + 1) * n] for blk in (v, Av, pb))
        A = [s8(b) for w in list(vr) + list(pr) for b in word_bytes(int(w))]
        words = []
        for Bt, start in img:
            kprime = len(Bt[0][0])
            row = []
            for col in range(16):
                total = 0
                for t in range(8):
                    acc = start[t][col]
                    lo, hi = min(lo, acc), max(hi, acc)
                    for k0 in range(0, kprime, 64):                 # one MFMA: 64 products
                        acc += sum(map(operator.mul, A[k0:k0 + 64], Bt[t][col][k0:k0 + 64]))
                        lo, hi = min(lo, acc), max(hi, acc)
                    assert -(1 << 31) <= lo and hi < 1 << 31
                    s_lo, s_hi = min(s_lo, acc), max(s_hi, acc)
                    total += (acc & 0xFFFFFFFF) << (8 * t)          # the kernel reads the accumulator as u32
                row.append((total + FCONST) % P)
            words.append(row)
        for j in range(n):
            dj = int(d[j]) != 0
            if n == 16:
                out_v.append((words[0][j] + int(ar[j] if dj else vr[j])) % P)
                out_p.append((words[1][j] + (0 if dj else int(pr[j]))) % P)
            else:
                out_v.append((words[0][j] + int(ar[j] if dj else vr[j])) % P)
                out_p.append((words[0][8 + j] + (0 if dj else int(pr[j]))) % P)
    return out_v, out_p, lo, hi, s_lo, s_hi


DOT_START = 1 << 30
W8 = sum(1 << (8 * a) for a in range(8)) % P
K1 = 128 * W8 % P
K2 = 16384 * W8 * W8 % P
BIASW = sum(DOT_START << ((8 * s) % 61) for s in range(15)) % P
_pair_cache = {}


def digit_pair_sums(x, y):
    """for s = 0..14 the sum over a + b = s of (byte a of x - 128)(byte b of y - 128): what ONE row adds to the 15
    accumulators of an entry whose operands are x and y"""
    got = _pair_cache.get((x, y))
    if got is None:
        xs, ys = [s8(b) for b in word_bytes(x)], [s8(b) for b in word_bytes(y)]
        got = [sum(xs[a] * ys[s - a] for a in range(8) if 0 <= s - a < 8) for s in range(15)]
        _pair_cache[(x, y)] = got
    return got


def _product(Xr, Yr, rows, nwaves, fold):
    """sum over the rows of X[r,i] Y[r,j] for 16-column operands (lists of rows) as k_block_dot_mfma computes it:
    (entries [i][j], lo, hi)"""
    ntiles = (rows + 63) // 64
    zero = (0,) * 16
    tile_cache = {}

    def tile_delta(t):
        xs = tuple(tuple(Xr[r]) if r < rows else zero for r in range(64 * t, 64 * t + 64))   # rows past the end: zero words
        ys = tuple(tuple(Yr[r]) if r < rows else zero for r in range(64 * t, 64 * t + 64))
        got = tile_cache.get((xs, ys))
        if got is None:
            got = [[[0] * 16 for _ in range(16)] for _ in range(15)]
            for (xr, yr), times in collections.Counter(zip(xs, ys)).items():
                for i in range(16):
                    for j in range(16):
                        ds = digit_pair_sums(xr[i], yr[j])
                        for s in range(15):
                            got[s][i][j] += times * ds[s]
            tile_cache[(xs, ys)] = got
        return got

    lo = hi = DOT_START
    total = [[0] * 16 for _ in range(16)]
    tiles_done = 0
    for wave in range(min(nwaves, max(ntiles, 1))):
        acc = [[[DOT_START] * 16 for _ in range(16)] for _ in range(15)]
        res = [[0] * 16 for _ in range(16)]
        pending = nflush = 0

        def flush():
            for i in range(16):
                for j in range(16):
                    for s in range(15):
                        assert 0 <= acc[s][i][j] < 1 << 32          # read as u32
                        res[i][j] += acc[s][i][j] << ((8 * s) % 61)
                        acc[s][i][j] = DOT_START

        for t in range(wave, ntiles, nwaves):
            dl = tile_delta(t)
            for s in range(15):
                for i in range(16):
                    a_, d_ = acc[s][i], dl[s][i]
                    for j in range(16):
                        a_[j] += d_[j]
                lo = min(lo, min(min(row) for row in acc[s]))
                hi = max(hi, max(max(row) for row in acc[s]))
            tiles_done += 1
            pending += 1
            if pending == fold:
                flush()
                nflush, pending = nflush + 1, 0
        if pending:
            flush()
            nflush += 1
        for i in range(16):
            for j in range(16):
                total[i][j] += res[i][j] - nflush * BIASW
    csx = [sum(Xr[r][i] for r in range(rows)) for i in range(16)]
    csy = [sum(Yr[r][j] for r in range(rows)) for j in range(16)]
    R = 64 * tiles_done
    return [[(total[i][j] + K1 * (csx[i] + csy[j]) - K2 * R) % P for j in range(16)] for i in range(16)], lo, hi


def model_dot(v, Av, rows, n, nwaves=1, fold=64):
    """(v^T Av, Av^T Av, lo, hi) as k_block_dot_mfma computes them, `nwaves` wavefronts taking the 64-row tiles in turn
    and folding their accumulators every `fold` tiles.  n = 16: two products; n = 8: one, X = Y = [V | Av], whose
    off-diagonal and lower-right blocks are the results.  lo / hi: the least and largest value an accumulator holds
    between tiles (every entry of the 16 x 16 tile, the ones not written out included)."""
    assert n in (8, 16)
    Vr = [[int(w) for w in v[r * n:(r + 1) * n]] for r in range(rows)]
    Ar = [[int(w) for w in Av[r * n:(r + 1) * n]] for r in range(rows)]
    if n == 16:
        a, lo0, hi0 = _product(Vr, Ar, rows, nwaves, fold)
        b, lo1, hi1 = _product(Ar, Ar, rows, nwaves, fold)
        return [w for row in a for w in row], [w for row in b for w in row], min(lo0, lo1), max(hi0, hi1)
    XY = [Vr[r] + Ar[r] for r in range(rows)]
    c, lo, hi = _product(XY, XY, rows, nwaves, fold)
    return ([c[i][8 + j] for i in range(8) for j in range(8)], [c[8 + i][8 + j] for i in range(8) for j in range(8)],
            lo, hi)


def const_pair_range(x, y, tiles=64):
    """(lo, hi) of the accumulators of an entry whose operands are the constant words x and y, after `tiles` full tiles"""
    ends = [DOT_START + 64 * tiles * q for q in digit_pair_sums(x, y)]
    return min(ends + [DOT_START]), max(ends + [DOT_START])


# what no pair of words below p can pass in 64 tiles: 8 digit pairs (s = 7) of (-128)(-128), or of (127)(-128)
DOT_HI_END = DOT_START + 64 * 64 * 8 * 128 * 128
DOT_LO_END = DOT_START - 64 * 64 * 8 * 128 * 127
# the update: S_t = 2^24 + sum over K' of (byte) * (signed digit), bytes 0..255, digits -128..127, K' = 16 n
UPDATE_HI_END = {n: ORTHO_START + 16 * n * 255 * 127 for n in (8, 16)}
UPDATE_LO_END = {n: ORTHO_START - 16 * n * 255 * 128 for n in (8, 16)}


# ------------------------------------------------------------------------------------------------ closed forms


def const_dot(a, b, rows, n):
    """V all a, Av all b: (v^T Av, Av^T Av), every entry rows a b and rows b^2 mod p"""
    return [rows * a * b % P] * (n * n), [rows * b * b % P] * (n * n)


def cycle_dot(rows, n, shift_v, shift_av):
    """V = cycle_block(rows, n, shift_v), Av = cycle_block(rows, n, shift_av): the sums over one period times the whole
    periods, plus the sums over the remainder"""
    q, rem = divmod(rows, L)

    def entry(u, w):
        per = sum(PATTERNS[(r + u) % L] * PATTERNS[(r + w) % L] for r in range(L))
        tail = sum(PATTERNS[(r + u) % L] * PATTERNS[(r + w) % L] for r in range(rem))
        return (q * per + tail) % P

    vtav = [entry(i + shift_v, j + shift_av) for i in range(n) for j in range(n)]
    vtaav = [entry(i + shift_av, j + shift_av) for i in range(n) for j in range(n)]
    return vtav, vtaav


def tiled_update(v_per, Av_per, p_per, d, S, B, winv, rows, n):
    """The update is row-local: exact_ref.orthogonalize on one period of rows (flat lists, the same number of rows each),
    repeated down to `rows` rows.  Returns (v', p') as flat uint64 arrays."""
    per = len(v_per) // n
    ev, ep = X.orthogonalize(v_per, p_per, d, S, B, winv, per, Av_per, n, P)
    out = []
    for e in (ev, ep):
        one = np.array(e, dtype=np.uint64).reshape(per, n)
        out.append(np.tile(one, (rows // per + 1, 1))[:rows].reshape(-1))
    return out[0], out[1]
