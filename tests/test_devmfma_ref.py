"""devmfma_ref.py held to plain integer arithmetic, and the accumulator ranges of the device block algebra's matrix-core
recombination (csrc/blz_devmfma.hip) derived from it.  CPU only, no library.

The start of the int32 accumulators is derived, not inherited: a digit sum is START + sum over K' of u d with u in [0, 255]
and d in [-128, 127], so it lies in [START - K' 255 128, START + K' 255 127]; START = 512 * 255 * 128 puts the lower end at 0
for the longest K' (four terms at n = 16) and the upper end at 512 * 255 * 255 < 2^25.  Here the model is (1) shown to be the
operation, (2) asked for the range its accumulators take on mfma_digits_ref.PATTERNS x PATTERNS at that longest K', and (3)
asked which (block word, coefficient) pairs come closest to the ends: the pairs tests/test_gpu_device_mfma.py runs on the GPU.

How close "closest" has to be.  No residue reaches the analytic ends: its top byte is at most 0x1F, and the block word with
seven bytes 0xFF has a zero top byte, which silences 64 of the 512 K' positions -- one matrix-core product (one
v_mfma_i32_16x16x64_i8, 64 products) of the chain's eight.  On the high side the worst pair must be within that one product's
worth, 64 * 255 * 127.  On the low side a coefficient's signed digits cannot all be -128: the recoding reaches -128 where a
carry chain starts and -127 along it, one unit of 255 per live position, so the allowance is 64 * 255 * 128 + 448 * 255.
(Measured: 2 072 640 above and 2 186 880 below, against allowances of 2 072 640 and 2 203 200.)
"""
import itertools

import pytest

import devmfma_ref as D
import mfma_digits_ref as R

P = R.P
NAMES = R.PATTERNS._fields
# the (block word, coefficient) pairs the search below finds (and asserts) as the worst of PATTERNS x PATTERNS
COMBINE_HIGHEST = ("ff_x7", "all_7f")
COMBINE_LOWEST = ("ff_x7", "all_80")


def test_the_start_is_derived_from_the_longest_contraction():
    assert D.KMAX == 512 and D.START == 512 * 255 * 128 == 16711680 and D.SUM_MAX == 512 * 255 * 255 < 1 << 25
    assert D.lo_end(16, 4) == 0 and D.hi_end(16, 4) == D.SUM_MAX
    for n in (8, 16):
        for nterms in (1, 2, 3, 4):
            assert 0 <= D.lo_end(n, nterms) and D.hi_end(n, nterms) <= D.SUM_MAX < 1 << 31
    # between two MFMAs an accumulator is start + 128 (sum of digits) + sum (u - 128) d: each part at most K' 128 128
    assert D.START + 2 * D.KMAX * 128 * 128 < 1 << 31 and D.START - 2 * D.KMAX * 128 * 128 > -(1 << 31)
    # the folded sums: eight digit sums below 2^25 with weights up to 2^24 in each of the two 64-bit halves
    assert 4 * (D.SUM_MAX << 24) < 1 << 56
    assert D.FCONST == (-sum(D.START << (8 * t) for t in range(8))) % P


def test_worst_pattern_pairs_at_four_terms_n16():
    n, nterms = 16, 4
    lows, highs = [], []
    for bn, cn in itertools.product(NAMES, NAMES):
        w, x = R.word(bn), R.word(cn)
        xs, a = [[w] * n] * nterms, [R.coef_const(x, n)] * nterms
        z0, z1, lo, hi, s_lo, s_hi = D.model_combine(xs, a, None, 1, n, cols=[0])       # every column is the same
        assert z1 is None and z0[0] == D.combine_exact(xs, a, 1, n)[0] == nterms * n * w * x % P, (bn, cn)
        assert 0 <= s_lo and s_hi < 1 << 32, (bn, cn)                                    # read as u32
        assert -(1 << 31) <= lo and hi < 1 << 31, (bn, cn)                               # int32 between MFMAs
        assert D.lo_end(n, nterms) <= s_lo and s_hi <= D.hi_end(n, nterms)
        lows.append((s_lo, bn, cn))
        highs.append((s_hi, bn, cn))
    low, high = min(lows), max(highs)
    print(f"S lowest {low[0]} at block {low[1]} x coefficient {low[2]}, highest {high[0]} at {high[1]} x {high[2]}; "
          f"no input passes [{D.lo_end(n, nterms)}, {D.hi_end(n, nterms)}]")
    assert low[1:] == COMBINE_LOWEST and high[1:] == COMBINE_HIGHEST
    live = D.kprime(n, nterms) - 64
    assert D.hi_end(n, nterms) - high[0] <= 64 * 255 * 127
    assert low[0] - D.lo_end(n, nterms) <= 64 * 255 * 128 + live * 255
    pm1 = [q for q in lows if q[1:] == ("pm1", "pm1")][0][0], [q for q in highs if q[1:] == ("pm1", "pm1")][0][0]
    span = D.hi_end(n, nterms) - D.lo_end(n, nterms)
    assert pm1[0] - D.lo_end(n, nterms) > 0.3 * span and D.hi_end(n, nterms) - pm1[1] > 0.3 * span, "all-(p-1) is near no end"


COEFS = {"const": lambda n, t: R.coef_const(R.word("top_80"), n), "cycle": lambda n, t: R.coef_cycle(n, 3 * t),
         "rotation": lambda n, t: R.coef_rotation(n)}


@pytest.mark.parametrize("maker", sorted(COEFS))
@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [8, 16])
def test_model_is_plain_integer_arithmetic_on_cycle_blocks(n, nterms, maker):
    rows = R.L if n == 8 else 4
    xs = [[w for row in R.cycle_period(n, 5 * t)[:rows] for w in row] for t in range(nterms)]
    a0 = [COEFS[maker](n, t) for t in range(nterms)]
    z0, z1, lo, hi, s_lo, s_hi = D.model_combine(xs, a0, None, rows, n)
    assert z1 is None and z0 == D.combine_exact(xs, a0, rows, n)
    assert D.lo_end(n, nterms) <= s_lo and s_hi <= D.hi_end(n, nterms) and -(1 << 31) <= lo and hi < 1 << 31


@pytest.mark.parametrize("n", [8, 16])
def test_model_of_the_pair_with_zero_panels(n):
    """Z0 | Z1 in the 16 tile columns at n = 8, two images at n = 16; a NULL coefficient is a zero panel"""
    rows = 3
    xs = [[w for row in R.cycle_period(n, 5 * t)[:rows] for w in row] for t in range(3)]
    a0 = [R.coef_cycle(n, 1), R.coef_rotation(n), R.coef_const(R.word("all_80"), n)]
    a1 = [None, R.coef_cycle(n, 7), R.coef_const(R.word("all_7f"), n)]
    z0, z1 = D.model_combine(xs, a0, a1, rows, n)[:2]
    assert z0 == D.combine_exact(xs, a0, rows, n) and z1 == D.combine_exact(xs, a1, rows, n)
    t = D.tiled(z0, 2 * rows + 1, n)
    assert t.shape == (2 * rows + 1, n) and t.reshape(-1).tolist() == (z0 * 3)[:(2 * rows + 1) * n]
