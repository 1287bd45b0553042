"""The matrix-core kernels (csrc/blz_dense_mfma.hip: k_ortho_mfma_prep, k_ortho_mfma, k_block_dot_mfma) against exact
integers at THEIR bounds, which are digit bounds (tests/mfma_digits_ref.py): the byte 0x00 that XOR 0x80 turns into -128,
the step from 0x7F to 0x80, the carries of the signed recoding of a coefficient, rotations of a coefficient that wrap,
and the re-start of the inner product's accumulators after 64 tiles.  tests/test_mfma_digits_ref.py derives which inputs
reach them; all-(p-1) blocks and random words, what the other matrix-core tests use, do not.

Every case runs at p = 2^61-1 with BLZ_NO_REORDER=1 and BLZ_MFMA_MIN_ROWS=0 (the update on the matrix cores at every row
count), and once more with BLZ_NO_MFMA=1 against the SAME expectation: if the vector-ALU kernels miss it too, the
expectation is what is wrong.  The expectations are exact_ref on one period of rows (the update is row-local) and closed
forms in Python integers (the inner products); no oracle pass.

A. the update at rows around the 16-row tile, coefficients chosen by their digits;
B. the inner products at rows around the 64-row tile (the rows that fill the last tile are zero words, bytes of -128,
   which the K2 * R term has to take out again);
C. the inner products with so many rows that EVERY wavefront folds its accumulators once at 64 tiles and once at the end.
"""
import functools

import numpy as np
import pytest

import blz
import exact_ref as X
import mfma_digits_ref as R
from test_gpu_exact import device_cus, tall

pytestmark = pytest.mark.gpu

P = R.P


def first_difference(got, want, n):
    at = np.flatnonzero(got != want)
    if not len(at):
        return None
    k = int(at[0])
    return dict(row=k // n, column=k % n, got=hex(int(got[k])), want=hex(int(want[k])), wrong_words=len(at))


def matrix_cores(monkeypatch, on, stage8=False):
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    monkeypatch.setenv("BLZ_NO_MFMA", "0" if on else "1")
    monkeypatch.setenv("BLZ_MFMA_STAGE8", "1" if stage8 else "0")


# ------------------------------------------------------------------------------------------------ A. the update


@functools.lru_cache(maxsize=None)
def update_cases(n):
    """(name, period of v, of Av, of p -- flat lists of whole rows --, VTAV, VTAAV, npiv, winv, d).

    blz_orthogonalize reads c and vtAvd from the panels the semi-inverse kernel writes (on every path: blz_set_small
    reaches vtAv, vtAAv, winv and d only), so no coefficient can be set directly: all of them come through semi_inverse
    of a triangular matrix, mfma_digits_ref.through_semi_inverse.  With d all ones c is the maker's matrix, vtAvd its
    upper triangle and winv minus the triangle's inverse; with d alternating, c's odd columns come from vtAv, vtAvd's are
    zero and the terms (d ? Av : v) and (d ? 0 : p) are live in both forms."""
    makers = {"const": R.coef_const(R.word("top_80"), n), "cycle": R.coef_cycle(n), "rotation": R.coef_rotation(n)}
    vtavd = {"const": makers["const"], "cycle": R.coef_cycle(n, 7), "rotation": makers["rotation"]}
    cyc = tuple([w for row in R.cycle_period(n, s) for w in row] for s in (0, 5, 11))
    out = []

    def add(name, blocks, C, T, mixed):
        S, B, _, _, want_d = R.through_semi_inverse(C, T, n, mixed)
        npiv, winv, d = X.semi_inverse(S, n, P)
        assert d == want_d
        out.append((name, blocks[0], blocks[1], blocks[2], S, B, npiv, winv, d))

    for name in makers:
        for mixed in (False, True):
            add(f"cycle blocks, {name} coefficients, d {'alternating' if mixed else 'all ones'}", cyc, makers[name],
                vtavd[name], mixed)
    # the constant pairs test_mfma_digits_ref.py names as the worst: (block word, coefficient) of the update's digit sums,
    # and the (v word, p word) that drive an inner product's accumulators to their ends, here as the two halves of K'
    for bn, cn in (R.UPDATE_HIGHEST, R.UPDATE_LOWEST):
        w = [R.word(bn)] * n
        add(f"blocks {bn}, coefficients {cn}", (w, [P - 1] * n, w), R.coef_const(R.word(cn), n), R.coef_const(R.word(cn), n), False)
    for an, bn in (R.DOT_HIGHEST, R.DOT_LOWEST):
        add(f"v {an}, p {bn}, rotation coefficients", ([R.word(an)] * n, [R.word(bn)] * n, [R.word(bn)] * n), makers["rotation"],
            makers["rotation"], True)
    return out


def rows_of(period, rows, n):
    one = np.array(period, dtype=np.uint64).reshape(-1, n)
    return np.tile(one, (rows // len(one) + 1, 1))[:rows].reshape(-1)


UPDATE_PARAMS = [(n, rows, st) for n in (8, 16) for rows in (1, 16, 17, 257, 4099) for st in ((0, 1) if n == 8 else (0,))]


@pytest.mark.parametrize("n,rows,stage8", UPDATE_PARAMS, ids=[f"n{n}-rows{r}-stage{s}" for n, r, s in UPDATE_PARAMS])
def test_update_at_the_digit_bounds(monkeypatch, n, rows, stage8):
    """Rows at the edges of the 16-row tile and two counts that give a wavefront several tiles; at n = 8 both the direct
    and the LDS-staged form (BLZ_MFMA_STAGE8).  Every word of V and P against exact_ref.orthogonalize."""
    for on in (True,) if stage8 else (True, False):
        matrix_cores(monkeypatch, on, bool(stage8))
        with blz.Context(P, n) as ctx:
            ctx.set_matrix(tall(rows), False)
            for name, v, Av, pb, S, B, npiv, winv, d in update_cases(n):
                for blk, per in ((blz.V, v), (blz.AV, Av), (blz.P, pb)):
                    ctx.set_block(blk, rows_of(per, rows, n))
                ctx.set_small(blz.VTAV, np.array(S, np.uint64))
                ctx.set_small(blz.VTAAV, np.array(B, np.uint64))
                got = ctx.semi_inverse()
                assert (got[0], [int(w) for w in got[1]], [int(w) for w in got[2]]) == (npiv, winv, d), (name, "semi_inverse")
                ctx.orthogonalize()
                ev, ep = R.tiled_update(v, Av, pb, d, S, B, winv, rows, n)
                where = "matrix cores" if on else "vector ALU"
                for which, blk, want in (("v", blz.V, ev), ("p", blz.P, ep)):
                    diff = first_difference(ctx.get_block(blk), want, n)
                    assert diff is None, (name, where, which, diff)


# ------------------------------------------------------------------------------------------------ B, C. inner products

CONST_PAIRS = (R.DOT_HIGHEST, R.DOT_LOWEST, R.DOT_LOWEST[::-1])
CYCLE_PAIRS = ((2, 9), (0, 0))


def check_dots(monkeypatch, n, rows, pairs):
    """pairs: ("const", name of V's word, name of Av's) or ("cycle", shift of V, shift of Av)"""
    for on in (True, False):
        matrix_cores(monkeypatch, on)
        with blz.Context(P, n) as ctx:
            ctx.set_matrix(tall(rows), False)
            for kind, a, b in pairs:
                if kind == "const":
                    ctx.set_block(blz.V, R.const_block(R.word(a), rows, n))
                    ctx.set_block(blz.AV, R.const_block(R.word(b), rows, n))
                    want = R.const_dot(R.word(a), R.word(b), rows, n)
                else:
                    ctx.set_block(blz.V, R.cycle_block(rows, n, a))
                    ctx.set_block(blz.AV, R.cycle_block(rows, n, b))
                    want = R.cycle_dot(rows, n, a, b)
                got = ctx.block_dot()
                where = "matrix cores" if on else "vector ALU"
                for which, g, w in (("vtAv", got[0], want[0]), ("vtAAv", got[1], want[1])):
                    diff = first_difference(g, np.array(w, np.uint64), n)
                    assert diff is None, (kind, a, b, where, which, diff)


@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("rows", [4096, 4097, 4159, 4160])
def test_inner_products_at_the_digit_bounds(monkeypatch, n, rows):
    """The 64-row tile's edges, from the first row count that takes the matrix cores (launch_block_dot: rows >= 4096)."""
    check_dots(monkeypatch, n, rows, [("const",) + q for q in CONST_PAIRS] + [("cycle",) + q for q in CYCLE_PAIRS])


def rows_past_the_fold():
    """launch_block_dot_mfma starts at most 2 * num_cu workgroups of DBLOCK / 64 = 4 wavefronts, which take the 64-row tiles
    in turn; with 65 tiles for every one of those W wavefronts, and one tile more, each wavefront folds its accumulators at
    pending == 64 and once more at the end (a smaller grid only gives a wavefront more tiles)."""
    W = 4 * 2 * device_cus()
    return 64 * 65 * W + 1


PAST_FOLD = [(8, ("const",) + R.DOT_HIGHEST), (8, ("const",) + R.DOT_LOWEST), (8, ("cycle", 2, 9)),
             (16, ("const",) + R.DOT_HIGHEST), (16, ("cycle", 2, 9))]


@pytest.mark.parametrize("n,pair", PAST_FOLD, ids=[f"n{n}-{'-'.join(str(q) for q in pair)}" for n, pair in PAST_FOLD])
def test_inner_products_past_the_fold(monkeypatch, n, pair):
    """What no other test of a few seconds reaches: the accumulators re-started after a flush, nflush = 2 in the bias term
    and the rows processed taken from the tile count, on the inputs that drive the accumulators to both ends of their range
    (2^30 + 2^29 and 2^30 - 2^29 + 2^22 after 64 tiles) and on cycle blocks.  8.5 M rows on 256 compute units; the expected
    words are closed forms."""
    rows = rows_past_the_fold()
    # V, AV, P and TMP of the context at 8 bytes a word, as in test_gpu_exact.py; 4.5 GB is what n = 16 takes on 256 CUs
    assert rows * n * 8 * 4 < 4.5e9
    check_dots(monkeypatch, n, rows, [pair])
