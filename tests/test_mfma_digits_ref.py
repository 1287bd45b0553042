"""mfma_digits_ref.py held to exact_ref, and the accumulator ranges of the matrix-core kernels derived from it.

The model restates what csrc/blz_dense_mfma.hip and csrc/ortho_img.h compute (bytes XOR 0x80, rot61, signed digits, the
accumulator starts, the folds and their correction terms) in Python integers.  Here it is (1) shown to give the words of
exact_ref.orthogonalize / exact_ref.block_dot on every pair of byte patterns, so that it IS the operation; (2) asked for
the range its int32 accumulators take, which is asserted against the bounds the kernels' comments state; and (3) asked
which inputs come closest to those bounds: the pairs tests/test_gpu_mfma_digits.py then runs on the GPU.  All-(p-1)
operands, the bound of every other kernel family, stay well inside: that is why these tests exist.
"""
import itertools

import pytest

import exact_ref as X
import mfma_digits_ref as R

P = R.P
NAMES = R.PATTERNS._fields


def test_patterns_are_residues_and_hold_the_byte_classes():
    assert all(0 <= w < P for w in R.PATTERNS) and len(set(R.PATTERNS)) == R.L
    for need in (0, 1, P - 1, 1 << 60, 0x00FFFFFFFFFFFFFF, 0x1F7F7F7F7F7F7F7F, 0x1F80808080808080, 0x0080808080808080,
                 0x007F7F7F7F7F7F7F, 0x00FF00FF00FF00FF, 0x1F00FF00FF00FF00, 0x1FFFFFFFFFFFFF7F, 0x80, 1 << 60):
        assert need in R.PATTERNS, hex(need)
    # every byte position below the top one sees 0x00, 0x7F, 0x80 and 0xFF; the top one 0x00 and 0x1F (its largest)
    for a in range(7):
        assert {0x00, 0x7F, 0x80, 0xFF} <= {R.word_bytes(w)[a] for w in R.PATTERNS}, a
    assert {0x00, 0x1F} <= {R.word_bytes(w)[7] for w in R.PATTERNS}
    # a block of them has no tile in which a column misses a pattern: the period is coprime to 16 and to 64
    assert R.L % 2 == 1


def test_signed_digits_and_rotations():
    """x = sum_t signed_digit(x, t) 256^t with every digit in [-128, 127] (a carry into the next digit wherever a byte is
    0x80 or more), and rot61(x, 8a) = x 2^(8a) mod p, on every pattern and every rotation of it."""
    carried = wrapped = 0
    for w in R.PATTERNS:
        for a in range(8):
            x = R.rot61(w, 8 * a)
            assert x == (w << (8 * a)) % P
            wrapped += (w << (8 * a)) >= 1 << 61
            ds = [R.signed_digit(x, t) for t in range(8)]
            assert all(-128 <= q <= 127 for q in ds) and sum(q << (8 * t) for t, q in enumerate(ds)) == x
            carried += any(q < 0 for q in ds)
    assert carried > 30 and wrapped > 30
    assert R.rot61(P - 1, 8) == P - 256 and R.rot61(1 << 60, 1) == 1


@pytest.mark.parametrize("n", [8, 16])
def test_update_model_is_the_update_on_every_pattern_pair(n):
    """Block word x coefficient word, one row each (the update is row-local); d alternates so that both forms of the
    term that is no product are taken.  Also the accumulator range of the whole set, against the kernel's comment
    ("keeps the digit sum S_t positive (< 2^25)"), and the pairs that come closest to its ends."""
    d = [j % 2 for j in range(n)]
    lows, highs = [], []
    for bn, cn in itertools.product(NAMES, NAMES):
        w, x = R.word(bn), R.word(cn)
        v, Av, pb = [w] * n, [(w + 1) % P] * n, [R.PATTERNS[(NAMES.index(bn) + 1) % R.L]] * n
        co = R.coef_const(x, n)
        gv, gp, lo, hi, s_lo, s_hi = R.model_update(v, Av, v, co, co, co, d, 1, n)      # v and p both the block word
        assert (gv, gp) == _update(v, Av, v, co, co, co, d, 1, n), (bn, cn)
        assert 0 < s_lo and s_hi < 1 << 25 and 0 < lo and hi < 1 << 25, (bn, cn, lo, hi)
        assert R.UPDATE_LO_END[n] <= s_lo and s_hi <= R.UPDATE_HI_END[n]
        lows.append((s_lo, bn, cn))
        highs.append((s_hi, bn, cn))
        if bn != "pm1":                                             # and once with a different word in p
            gv, gp = R.model_update(v, Av, pb, co, co, co, d, 1, n)[:2]
            assert (gv, gp) == _update(v, Av, pb, co, co, co, d, 1, n), (bn, cn, "p")
    lo_end, hi_end = R.UPDATE_LO_END[n], R.UPDATE_HI_END[n]
    assert 0 < lo_end and hi_end < 1 << 25                          # no input at all can leave (0, 2^25)
    low, high = min(lows), max(highs)
    print(f"n={n}: S_t lowest {low[0]} at block {low[1]} x coefficient {low[2]}, highest {high[0]} at {high[1]} x {high[2]}"
          f"; no input passes [{lo_end}, {hi_end}]")
    assert low[1:] == R.UPDATE_LOWEST and high[1:] == R.UPDATE_HIGHEST
    # the worst pairs of the set cover most of what any input can reach; all-(p-1) stays in the middle
    span = hi_end - lo_end
    assert low[0] - lo_end < 0.15 * span and hi_end - high[0] < 0.15 * span
    pm1_lo = [q for q in lows if q[1:] == ("pm1", "pm1")][0][0]
    pm1_hi = [q for q in highs if q[1:] == ("pm1", "pm1")][0][0]
    assert pm1_lo - lo_end > 0.02 * span and hi_end - pm1_hi > 0.02 * span
    assert pm1_lo - lo_end > 0.4 * span and hi_end - pm1_hi > 0.3 * span, "all-(p-1) is nowhere near a digit bound"


def _update(v, Av, pb, c, vd, winv, d, rows, n):
    """exact_ref.orthogonalize's sums with c and vtAvd given directly (ortho_coeffs left out)"""
    out_v, out_p = [], []
    for r in range(rows):
        vr, ar, pr = (b[r * n:(r + 1) * n] for b in (v, Av, pb))
        for j in range(n):
            out_v.append(((ar[j] if d[j] else vr[j]) + sum(vr[k] * c[k * n + j] + pr[k] * vd[k * n + j] for k in range(n))) % P)
            out_p.append(((0 if d[j] else pr[j]) + sum(vr[k] * winv[k * n + j] for k in range(n))) % P)
    return out_v, out_p


COEF_MAKERS = {"const": lambda n: R.coef_const(R.word("all_7f"), n), "cycle": lambda n: R.coef_cycle(n),
               "rotation": R.coef_rotation}


@pytest.mark.parametrize("mixed", [False, True], ids=["d_ones", "d_mixed"])
@pytest.mark.parametrize("maker", sorted(COEF_MAKERS))
@pytest.mark.parametrize("n", [8, 16])
def test_update_model_on_cycle_blocks_with_coefficients_through_semi_inverse(n, maker, mixed):
    """The inputs of the GPU cases: through_semi_inverse gives VTAV and VTAAV whose semi-inverse and ortho_coeffs are the
    chosen c and vtAvd (exact_ref says so), and on one period of cycle blocks the model equals exact_ref.orthogonalize."""
    C = COEF_MAKERS[maker](n)
    S, B, want_c, want_vd, want_d = R.through_semi_inverse(C, C, n, mixed)
    npiv, winv, d = X.semi_inverse(S, n, P)
    assert d == want_d and npiv == sum(want_d)
    c, vd = X.ortho_coeffs(S, B, winv, d, n, P)
    assert vd == want_vd
    assert all(c[k * n + j] == want_c[k * n + j] for k in range(n) for j in range(n) if d[j])
    if mixed:
        assert any(c[k * n + j] for k in range(n) for j in range(n) if not d[j]), "the columns of c from vtAv are live"
    else:
        assert c == C
    rows = R.L if n == 8 else 5
    v, Av, pb = ([w for row in R.cycle_period(n, s)[:rows] for w in row] for s in (0, 5, 11))
    gv, gp, lo, hi, _, _ = R.model_update(v, Av, pb, c, vd, winv, d, rows, n)
    assert (gv, gp) == X.orthogonalize(v, pb, d, S, B, winv, rows, Av, n, P)
    assert 0 < lo and hi < 1 << 25
    ev, ep = R.tiled_update(v, Av, pb, d, S, B, winv, 2 * rows + 3, n)
    assert ev.tolist() == (gv * 3)[:(2 * rows + 3) * n] and ep.tolist() == (gp * 3)[:(2 * rows + 3) * n]


@pytest.mark.parametrize("n", [8, 16])
def test_dot_model_is_the_inner_product_on_every_pattern_pair(n):
    """V all a, Av all b on 3 rows (61 zero rows fill the tile: their bytes are -128 and K2 * R takes them out again),
    against exact_ref.block_dot and the closed form."""
    rows = 3
    for an, bn in itertools.product(NAMES, NAMES):
        a, b = R.word(an), R.word(bn)
        v, Av = [a] * (rows * n), [b] * (rows * n)
        got = R.model_dot(v, Av, rows, n)
        assert got[:2] == X.block_dot(rows, Av, v, n, P) == R.const_dot(a, b, rows, n), (an, bn)
        assert 0 <= got[2] and got[3] < 1 << 32


@pytest.mark.parametrize("n,rows,nwaves,fold", [(8, 200, 1, 2), (8, 321, 2, 1), (16, 130, 2, 1), (8, 129, 3, 64)])
def test_dot_model_on_cycle_blocks_with_several_flushes(n, rows, nwaves, fold):
    """Cycle blocks over several tiles, wavefronts and flushes (the re-start of the accumulators, nflush > 1 in the bias
    term, the rows processed from the tile count, a last tile partly past the end) against exact_ref.block_dot; the
    closed form of cycle_dot equals both."""
    v, Av = R.cycle_block(rows, n, 2).tolist(), R.cycle_block(rows, n, 9).tolist()
    got = R.model_dot(v, Av, rows, n, nwaves=nwaves, fold=fold)
    want = X.block_dot(rows, Av, v, n, P)
    assert got[:2] == want
    assert R.cycle_dot(rows, n, 2, 9) == want


def test_cycle_and_const_blocks():
    b = R.cycle_block(40, 8, 3).reshape(40, 8)
    assert all(int(b[r, k]) == R.PATTERNS[(r + k + 3) % R.L] for r in range(40) for k in range(8))
    assert (R.const_block(5, 7, 16) == 5).all() and R.const_block(5, 7, 16).size == 112
    for rows in (1, R.L, 4096, 4097):
        assert R.cycle_dot(rows, 8, 0, 4) == X.block_dot(rows, R.cycle_block(rows, 8, 4).tolist(),
                                                         R.cycle_block(rows, 8, 0).tolist(), 8, P), rows


def test_inner_product_accumulators_over_one_fold_interval():
    """64 tiles (4096 rows) of every constant pair: each accumulator stays in [0, 2^32) -- in fact in [2^29, 3 * 2^29], as
    the kernel's comment says -- and the set holds the pairs that reach the ends no words below p can pass: zero bytes
    against zero bytes, 64 * 8 * 64 * 128^2 = 2^29 over the 2^30 start, and zero bytes against 0xFF bytes in all eight digit
    pairs of s = 7.  All-(p-1) stays 7 % of the range below the top.  The model itself, run over the 64 tiles, agrees."""
    assert R.DOT_HI_END == (1 << 30) + (1 << 29) and R.DOT_LO_END > 1 << 29
    ranges = {(an, bn): R.const_pair_range(R.word(an), R.word(bn)) for an, bn in itertools.product(NAMES, NAMES)}
    for pair, (lo, hi) in ranges.items():
        assert 0 <= R.DOT_LO_END <= lo and hi <= R.DOT_HI_END < 1 << 32, pair
    highest = max(ranges, key=lambda k: ranges[k][1])
    bottom = min(lo for lo, _ in ranges.values())
    lowest = sorted(k for k in ranges if ranges[k][0] == bottom)     # (alt_ff, alt_ff) reaches it too: FF against 00 by parity
    print(f"highest {ranges[highest][1]} at {highest}, lowest {bottom} at {lowest}; "
          f"no words pass [{R.DOT_LO_END}, {R.DOT_HI_END}]")
    assert highest == R.DOT_HIGHEST and ranges[highest][1] == R.DOT_HI_END
    assert R.DOT_LOWEST in lowest and bottom == R.DOT_LO_END
    span = R.DOT_HI_END - R.DOT_LO_END
    lo, hi = ranges[("pm1", "pm1")]
    assert lo - R.DOT_LO_END > 0.02 * span and R.DOT_HI_END - hi > 0.02 * span
    # the model over 64 tiles and one more (one flush at 64, one at the end), n = 8: V and Av of the two worst pairs
    rows = 64 * 65
    for an, bn in (R.DOT_HIGHEST, R.DOT_LOWEST, ("pm1", "pm1")):
        a, b = R.word(an), R.word(bn)
        got = R.model_dot([a] * (rows * 8), [b] * (rows * 8), rows, 8)
        assert got[:2] == R.const_dot(a, b, rows, 8)
        pairs = [ranges[q] for q in ((an, an), (an, bn), (bn, an), (bn, bn))]       # X = Y = [V | Av]: all four meet
        assert (got[2], got[3]) == (min(q[0] for q in pairs), max(q[1] for q in pairs))
    # without a fold the lowest pair leaves the u32 (below 0) at 130 tiles, the highest (2^32) at 384: the interval of 64
    # has a factor 2 in hand, and no GPU case of a few seconds can show a longer one failing -- it rests on this model
    low = (R.word(R.DOT_LOWEST[0]), R.word(R.DOT_LOWEST[1]))
    assert R.const_pair_range(*low, tiles=130)[0] < 0 <= R.const_pair_range(*low, tiles=129)[0]
    assert R.const_pair_range(0, 0, tiles=384)[1] >= 1 << 32 > R.const_pair_range(0, 0, tiles=383)[1]
