"""The device block algebra (csrc/blz_devalg.hip, blz_devsmall.hip) against exact integers at every reducer
class of csrc/modp.h and at the widths 1 ... 64: the ladder tests/test_gpu_exact.py holds the solver's own kernels to, for
the calls on caller-owned blocks -- Context.dot, dot_pair, combine, combine_pair, semi_inverse_device, ortho_coeffs, rref.

tests/device_exact.py restates what the launchers decide (tile rows, workgroups, slices, lane groups, threads, which panels
sit in LDS) and holds the case lists; tests/test_device_exact_host.py holds those to the kernels' table of forms and shows,
on a model of reduce128<0>, where the inputs below are a wrong word if a sum takes a product too many.

A. random residues with 0 and p - 1 planted, against Python integers (the oracle's block_dot above 300 000 products): every
   width of FULL_WIDTHS at 2^57 - 13 and 2^61 - 1, widths 2, 8, 24, 64 at the other new primes (2^32 - 5, the last prime of the
   96-bit accumulators; 2^32 + 15, the first of 8-byte words; the largest of 48, 56, 58, 59, 60 bits); row counts around the
   tile, every stride form, every aliasing pattern and in-place form, 1 ... 4 terms;
B. dot and dot_pair on all-(p-1) blocks of dot_rows_past_chunk rows: every accumulator of the launch takes chunk + 2 products;
C. combine and combine_pair with every word and coefficient p - 1 and terms * n >= chunk + 2;
D. semi_inverse_device and ortho_coeffs on every n x n kind of exact_ref and on the inverse of -(J + I), whose coefficient
   products are n products of (p-1)^2 per word; rref on random blocks at every width and on the echelon whose reduction
   takes n - 1 products of (p-1)^2 per word;
E. one iteration rebuilt from the four fused calls per new class, against blz_iterate on a twin.

Every comparison is equality of u64 words.  A kernel that lets chunk + 1 products into a sum fails B and C at 57 bits; one that
lets chunk + 2 in fails them at every Barrett prime of 57 ... 62 bits.
"""
import numpy as np
import pytest
import torch

import blz
import device_exact as DX
import exact_ref as X
import kbasis_ref as kb
import oracle as orc
import test_gpu_device_fused as F
from test_gpu_device_small import check_rref, info_of, panels_ref, rref_blocks
from test_gpu_exact import device_cus, expect_semi, ones_echelon

pytestmark = pytest.mark.gpu

assert F.MASKS == DX.MASKS and F.PADS == DX.PADS
DEV = F.DEV
PY_PRODUCTS = 300000                                    # Python integers up to here, per product of two blocks
_CUS = []


def cus():
    if not _CUS:
        _CUS.append(device_cus())
    return _CUS[0]


def case_id(*case):
    return "-".join(DX.pid(v) if v > 64 else f"n{v}" for v in case[:2]) + "".join(f"-t{v}" for v in case[2:])


def ids(cases):
    return [case_id(*c) for c in cases]


def same(t, want):
    return np.array_equal(F.to_host(t), want)


def full(shape, p, pad=0):
    """all words p - 1, made on the device; (view of the first n columns, base)"""
    base = torch.full((shape[0], shape[1] + pad), p - 1, dtype=torch.int64, device=DEV)
    return base[:, :shape[1]], base


# ------------------------------------------------------------------------------------------ A. random residues


def exact_gram(Xw, Yw, p, n):
    rows = Xw.shape[0]
    if rows * n * n <= PY_PRODUCTS:
        return F.gram_ref(Xw, Yw, p, n)
    return orc.block_dot(rows, F.flat(Yw), F.flat(Xw), n, p)[0].reshape(n, n)


@pytest.mark.parametrize("p, n", DX.RANDOM_CASES + DX.DOT_EXTRA, ids=ids(DX.RANDOM_CASES + DX.DOT_EXTRA))
def test_dot_and_dot_pair_against_exact_integers(p, n):
    with blz.Context(p, n) as ctx:                      # no matrix: the rows are the caller's
        for rows in DX.dot_rows(n):
            H = {k: F.residues(rows, n, p, s) for k, s in (("A", 1), ("B", 2), ("Y", 3))}
            exact = {k: exact_gram(W, H["Y"], p, n) for k, W in H.items()}          # once per row count
            gram_a = exact_gram(H["A"], H["A"], p, n)
            assert np.array_equal(exact["Y"], exact["Y"].T)
            for pads in DX.DOT_PADS:
                devs = {k: F.to_dev(H[k], pad) for k, pad in zip("ABY", pads)}
                T = {k: v[0] for k, v in devs.items()}
                tag = (rows, pads)
                c = ctx.dot(T["A"], T["Y"])
                assert c.dtype == torch.uint64 and tuple(c.shape) == (n, n) and same(c, exact["A"]), tag
                out = F.sentinel(n, n)                  # the caller's out, every word of it written
                assert ctx.dot(T["B"], T["Y"], out=out) is out and same(out, exact["B"]), tag
                assert same(ctx.dot(T["A"], T["A"]), gram_a) and same(ctx.dot(T["Y"], T["Y"]), exact["Y"]), tag + ("x is y",)
                # the five aliasing patterns: all distinct, x1 = y, x0 = y, x0 = x1, all the same
                for name, k0, k1 in (("distinct", "A", "B"), ("x1 is y", "A", "Y"), ("x0 is y", "Y", "B"), ("x0 is x1", "A", "A"),
                                     ("all one", "Y", "Y")):
                    got = F.to_host(ctx.dot_pair(T[k0], T[k1], T["Y"]))
                    assert got.shape == (2, n, n), tag
                    assert np.array_equal(got[0], exact[k0]) and np.array_equal(got[1], exact[k1]), tag + (name,)
                out = F.sentinel(2, n, n)
                assert ctx.dot_pair(T["A"], T["B"], T["Y"], out=out) is out
                assert np.array_equal(F.to_host(out)[0], exact["A"]) and np.array_equal(F.to_host(out)[1], exact["B"]), tag
                for k, (v, base) in devs.items():       # the inputs and their padding as they were
                    assert F.padding_intact(base, n) and same(v, H[k]), tag


class Products:
    """X_s A_t on Python integers, each computed once for the test that holds this"""

    def __init__(self, p, n, rows):
        self.p, self.n, self.rows, self.made = p, n, rows, {}

    def block(self, sx):
        return F.residues(self.rows, self.n, self.p, sx)

    def of(self, sx, sa):
        if (sx, sa) not in self.made:
            self.made[(sx, sa)] = F.obj(self.block(sx)) @ F.obj(F.coefficient(self.n, self.p, sa))
        return self.made[(sx, sa)]

    def want(self, pairs):
        z = np.zeros((self.rows, self.n), dtype=object)
        for sx, sa in pairs:
            z = z + self.of(sx, sa)
        return F.words(z % self.p).reshape(self.rows, self.n)


def as_coefficient(A, k):
    """a tensor, a numpy array or a nested list of Python integers, in turn"""
    return F.up(A) if k % 3 == 0 else A if k % 3 == 1 else A.tolist()


def combine_case(ctx, P, nterms, pads):
    p, n, rows = P.p, P.n, P.rows
    tag = (rows, nterms, pads)
    Xs = [P.block(10 + t) for t in range(nterms)]
    As = [F.coefficient(n, p, 20 + t) for t in range(nterms)]
    want = P.want([(10 + t, 20 + t) for t in range(nterms)])
    devs = [F.to_dev(Xw, pads[t % len(pads)]) for t, Xw in enumerate(Xs)]
    terms = [(devs[t][0], as_coefficient(As[t], t)) for t in range(nterms)]
    z = ctx.combine(terms)
    assert z.dtype == torch.uint64 and tuple(z.shape) == (rows, n) and same(z, want), tag
    out, base = F.to_dev(np.full((rows, n), F.SENTINEL, dtype=np.uint64), 3)        # the caller's strided out
    assert ctx.combine(terms, out=out) is out and same(out, want) and F.padding_intact(base, n), tag
    for t in range(nterms):                             # the inputs and their padding as they were
        assert same(devs[t][0], Xs[t]) and F.padding_intact(devs[t][1], n), tag
    last = devs[-1][0]                                  # in place on the last block: its own stride, its padding untouched
    assert ctx.combine(terms, out=last) is last and same(last, want) and F.padding_intact(devs[-1][1], n), tag + ("in place",)
    if nterms >= 2:                                     # the same block given as two terms, into a new block and in place
        xv, xb = F.to_dev(Xs[0], pads[0])
        twice = [(xv, As[0]), (xv, As[1])] + [(F.to_dev(Xs[t], pads[t % len(pads)])[0], As[t]) for t in range(2, nterms)]
        want2 = P.want([(10, 20), (10, 21)] + [(10 + t, 20 + t) for t in range(2, nterms)])
        assert same(ctx.combine(twice), want2), tag + ("one block twice",)
        assert ctx.combine(twice, out=xv) is xv and same(xv, want2) and F.padding_intact(xb, n), tag + ("one block twice, in place",)


COMBINE_CASES = DX.RANDOM_CASES + DX.COMBINE_EXTRA


@pytest.mark.parametrize("p, n", COMBINE_CASES, ids=ids(COMBINE_CASES))
def test_combine_against_exact_integers(p, n):
    """1 ... 4 terms at every stride form: at n = 48 two terms are the 256-thread launch and three the 1024-thread one"""
    with blz.Context(p, n) as ctx:
        for rows in DX.combine_rows(n):
            P = Products(p, n, rows)
            for nterms, pads in DX.combine_plan(n):
                combine_case(ctx, P, nterms, pads)


def pair_case(ctx, P, masks, pads):
    """combine_pair as tests/test_gpu_device_fused.py::combine_pair_case runs it, against Python integers throughout"""
    p, n, rows = P.p, P.n, P.rows
    nterms, tag = len(masks), (rows, masks, pads)
    Xs = [P.block(10 + t) for t in range(nterms)]
    A0 = [F.coefficient(n, p, 20 + t) if m[0] else None for t, m in enumerate(masks)]
    A1 = [F.coefficient(n, p, 30 + t) if m[1] else None for t, m in enumerate(masks)]
    w0 = P.want([(10 + t, 20 + t) for t, m in enumerate(masks) if m[0]])
    w1 = P.want([(10 + t, 30 + t) for t, m in enumerate(masks) if m[1]])

    def fresh():
        return [F.to_dev(Xw, pads[t % len(pads)]) for t, Xw in enumerate(Xs)]

    def terms_of(devs, kind=0):
        conv = lambda A, t: None if A is None else as_coefficient(A, t + kind)      # noqa: E731
        return [(devs[t][0], conv(A0[t], t), conv(A1[t], t)) for t in range(nterms)]

    devs = fresh()
    z0, z1 = ctx.combine_pair(terms_of(devs))           # z0 and z1 new blocks
    assert z0.dtype == z1.dtype == torch.uint64 and tuple(z0.shape) == tuple(z1.shape) == (rows, n)
    assert same(z0, w0) and same(z1, w1), tag
    (o0, b0), (o1, b1) = (F.to_dev(np.full((rows, n), F.SENTINEL, dtype=np.uint64), pad) for pad in (3, 2))
    got = ctx.combine_pair(terms_of(devs, 1), out=(o0, o1))                     # the caller's strided outputs
    assert got[0] is o0 and got[1] is o1 and same(o0, w0) and same(o1, w1), tag
    assert F.padding_intact(b0, n) and F.padding_intact(b1, n)
    for t in range(nterms):                             # the inputs and their padding as they were
        assert same(devs[t][0], Xs[t]) and F.padding_intact(devs[t][1], n), tag
    devs, z1 = fresh(), F.sentinel(rows, n)             # z0 in place on the last term, z1 new
    ctx.combine_pair(terms_of(devs, 2), out=(devs[-1][0], z1))
    assert same(devs[-1][0], w0) and same(z1, w1) and F.padding_intact(devs[-1][1], n), tag + ("z0 in place",)
    devs, z0 = fresh(), F.sentinel(rows, n)             # z1 in place on the first term, z0 new
    ctx.combine_pair(terms_of(devs), out=(z0, devs[0][0]))
    assert same(z0, w0) and same(devs[0][0], w1) and F.padding_intact(devs[0][1], n), tag + ("z1 in place",)
    if nterms >= 2:                                     # both in place on different terms: the Lanczos pattern
        devs = fresh()
        ctx.combine_pair(terms_of(devs, 1), out=(devs[-2][0], devs[-1][0]))
        assert same(devs[-2][0], w0) and same(devs[-1][0], w1), tag + ("both in place",)
        assert F.padding_intact(devs[-2][1], n) and F.padding_intact(devs[-1][1], n)
        assert all(same(devs[t][0], Xs[t]) for t in range(nterms - 2))


@pytest.mark.parametrize("p, n", COMBINE_CASES, ids=ids(COMBINE_CASES))
def test_combine_pair_against_exact_integers(p, n):
    """the MASKS of the fused file at every stride form; from n = 33 on also the panel counts of its n = 64 test: five panels
    are the LDS of a CU at n = 64, eight do not fit and the terms left over read theirs from global memory"""
    with blz.Context(p, n) as ctx:
        for rows in DX.combine_rows(n):
            P = Products(p, n, rows)
            for masks, pads in DX.pair_plan(n):
                pair_case(ctx, P, masks, pads)


# ------------------------------------------------------------------------------------------ B. dots past the chunk


@pytest.mark.parametrize("p, n", DX.DOT_PAST, ids=ids(DX.DOT_PAST))
def test_dots_past_the_chunk(p, n):
    """all words p - 1 on dot_rows_past_chunk rows: every accumulator of the launch takes at least chunk + 2 products, every
    product is (p-1)^2 = 1 mod p, and every entry is rows mod p.  An accumulator that took chunk + 1 products before a reduction
    gives a wrong word at 2^57 - 13, one that took chunk + 2 at every Barrett prime here (test_device_exact_host.py)."""
    rows = DX.dot_rows_past_chunk(p, n, cus())
    assert DX.dot_products_per_accumulator(rows, n, cus()) >= X.chunk(p) + 2
    want = np.full((n, n), rows % p, dtype=np.uint64)
    pair = np.stack([want, want])
    with blz.Context(p, n) as ctx:
        x, y, z = (full((rows, n), p)[0] for _ in range(3))
        assert same(ctx.dot(x, x), want), "x is y"
        assert same(ctx.dot(x, y), want), "x is not y"
        assert same(ctx.dot_pair(x, y, z), pair), "three blocks"
        assert same(ctx.dot_pair(x, x, x), pair), "one block"
        assert same(ctx.dot_pair(x, y, y), pair), "x1 is y"
        del y, z
        ys = full((rows, n), p, 1)[0]                   # a stride of n + 1 words: 8-byte lanes
        assert same(ctx.dot(x, ys), want) and same(ctx.dot(ys, ys), want), "8-byte lanes"
        assert same(ctx.dot_pair(ys, x, ys), pair) and same(ctx.dot_pair(ys, ys, ys), pair), "8-byte lanes"


# ------------------------------------------------------------------------------------------ C. combines past the chunk


@pytest.mark.parametrize("p, n, terms", DX.COMBINE_PAST, ids=ids(DX.COMBINE_PAST))
def test_combines_past_the_chunk(p, n, terms):
    """every block word and every coefficient is p - 1: a word of an output is n times the terms that enter it, a sum of
    terms * n >= chunk + 2 products of (p-1)^2.  In combine_pair the first term enters z0 only: the two outputs share one count,
    and the runs of chunk - cnt products (combine2_term) start in the middle of it -- at n = 5 and n = 6 runs of odd and of
    even length and the single trailing product (test_device_exact_host.py)."""
    rows, masks = 300, DX.past_masks(terms)
    in0, in1 = (sum(m[o] for m in masks) for o in (0, 1))
    word = lambda k: np.full((rows, n), k * n % p, dtype=np.uint64)              # noqa: E731
    with blz.Context(p, n) as ctx:
        a = torch.full((n, n), p - 1, dtype=torch.int64, device=DEV)
        for pad in (0, 3):                              # 16-byte lanes where n is even, 8-byte lanes

            def blocks():
                return [full((rows, n), p, pad) for _ in range(terms)]

            def triples(xs):
                return [(x, a if m[0] else None, a if m[1] else None) for (x, _), m in zip(xs, masks)]

            xs = blocks()
            assert same(ctx.combine([(x, a) for x, _ in xs]), word(terms)), pad
            z0, z1 = ctx.combine_pair(triples(xs))
            assert same(z0, word(in0)) and same(z1, word(in1)), pad
            ctx.combine([(x, a) for x, _ in xs], out=xs[-1][0])                 # in place
            assert same(xs[-1][0], word(terms)) and (F.to_host(xs[-1][1])[:, n:] == np.uint64(p - 1)).all(), (pad, "in place")
            xs = blocks()
            out = (xs[0][0], xs[-1][0]) if terms >= 2 else (xs[0][0], F.sentinel(rows, n))
            ctx.combine_pair(triples(xs), out=out)
            assert same(out[0], word(in0)) and same(out[1], word(in1)), (pad, "pair in place")
            assert all((F.to_host(base)[:, n:] == np.uint64(p - 1)).all() for _, base in xs), (pad, "padding")


# ------------------------------------------------------------------------------------------ D. small algebra


def square(A, n):
    return F.up(np.array(A, dtype=np.uint64).reshape(n, n))


@pytest.mark.parametrize("p, n", DX.SMALL_CASES, ids=ids(DX.SMALL_CASES))
def test_semi_inverse_and_ortho_coeffs_against_exact_integers(p, n):
    """k_dev_chain at 64, 256 and 1024 threads (lg = 5 and lg = 6) on every n x n kind of exact_ref, the non-symmetric ones
    included; the coefficient products W * S take n products per word with the chunk rule"""
    other = X.square_case("nonsym", n, p, seed=1)
    with blz.Context(p, n) as ctx:
        for kind in X.SQUARE_KINDS + X.NONSYM_KINDS:
            A = X.square_case(kind, n, p)
            npiv, winv, d = expect_semi(A, n, p)
            a = square(A, n)
            w, dd, k = ctx.semi_inverse_device(a)
            assert int(F.to_host(k)[0]) == npiv, kind
            assert F.to_host(dd).tolist() == list(d) and F.to_host(w).reshape(-1).tolist() == list(winv), kind
            B = X.square_case("all_max", n, p) if kind == "all_max" else other     # all p - 1 on both sides once
            want = panels_ref(A, B, winv, d, n, p)
            coef, k = ctx.ortho_coeffs(a, square(B, n))
            assert int(F.to_host(k)[0]) == npiv and same(coef, want), kind
            assert same(a, np.array(A, dtype=np.uint64).reshape(n, n)), kind       # the input as it was


@pytest.mark.parametrize("p, n", DX.CHAIN_PAST, ids=ids(DX.CHAIN_PAST))
def test_coefficients_past_the_chunk(p, n):
    """vtav = J / (n + 1) - I, whose inverse is W = -(J + I): p - 2 on the diagonal, p - 1 elsewhere, d all ones; vtaav all
    p - 1.  A word of W * S in k_dev_chain is then a sum of n - 1 products of (p-1)^2 and one of (p-2)(p-1), n >= chunk + 2 of
    them: two too many in one sum is a wrong word at each of these primes (test_device_exact_host.py).  No width reaches
    chunk + 2 = 66 at 57 bits."""
    assert (n + 1) % p and n >= X.chunk(p) + 2
    inv = pow(n + 1, -1, p)
    A = [(inv - (i == j)) % p for i in range(n) for j in range(n)]
    W = [p - 2 if i == j else p - 1 for i in range(n) for j in range(n)]
    B = [p - 1] * (n * n)
    npiv, winv, d = expect_semi(A, n, p)
    assert npiv == n and list(winv) == W and list(d) == [1] * n
    want = panels_ref(A, B, winv, d, n, p)
    assert (want[1] == np.uint64(-((n - 1) * (p - 1) ** 2 + (p - 2) * (p - 1)) % p)).all()      # (I - D) - W * S, D = I
    with blz.Context(p, n) as ctx:
        w, dd, k = ctx.semi_inverse_device(square(A, n))
        assert int(F.to_host(k)[0]) == n and F.to_host(dd).tolist() == [1] * n and F.to_host(w).reshape(-1).tolist() == W
        coef, k = ctx.ortho_coeffs(square(A, n), square(B, n))
        assert int(F.to_host(k)[0]) == n and same(coef, want)


@pytest.mark.parametrize("p, n", DX.RREF_RANDOM, ids=ids(DX.RREF_RANDOM))
def test_rref_of_random_blocks_at_every_width(p, n):
    """the blocks of tests/test_gpu_device_small.py (dense, repeated and zero columns, repeated rows, nothing new after the
    first n rows, a planted echelon of half rank, zero) at the widths and the 57-bit prime that file leaves out, against the
    elimination on Python integers: both strides, the null basis, e * z = 0"""
    rng = np.random.default_rng([p % 1000003, n, 29])
    with blz.Context(p, n) as ctx:
        for R in DX.rref_random_rows(n):
            for name, Xb in rref_blocks(rng, p, n, R).items():
                E, r, piv = kb.rref(Xb.tolist(), p, n)
                check_rref(ctx, Xb, p, n, E, r, list(piv), (R, name))


@pytest.mark.parametrize("p, n", DX.RREF_CASES, ids=ids(DX.RREF_CASES))
def test_rref_where_the_reduction_is_longest(p, n):
    """The distinct rows are (p-1) [I | 1], n - 1 of them, and (p-1) times their sum.  A workgroup of the partial pass takes
    every (2 * CUs)-th tile, so the block is laid out by tiles: each workgroup first meets the echelon rows (one tile of them
    up to n = 33, two at n = 48 and 64, where a tile has 32 rows), then a tile of sum rows, and the five rows at the end are sum
    rows too: 2 * (2 * CUs) * TR + 5 rows, a tile more per workgroup at the two widest.  A sum row then meets an echelon of rank
    n - 1, and its last word is reduced by n - 1 products of (p-1)^2.  RREF_PAST has n - 1 >= chunk + 2.  At 57 bits no width
    can pass the chunk (n - 1 <= 63 < 66), and at 2^61 - 1 none to the point of showing (64 products fit): RREF_VALUES runs
    those for the values, and the lane groups of 1 and 2 lanes."""
    TR, grid = DX.rref_tile_rows(n), 2 * cus()
    pattern = ones_echelon(n, p)
    echelon, total = pattern[:-1], pattern[-1]
    E, r, piv = kb.rref(pattern, p, n)
    assert r == n - 1
    Z = F.words(kb.null_basis(E, r, piv, n, p)).reshape(n, n)
    E = F.words(E).reshape(n, n)
    tiles = [(echelon[i:i + TR] * TR)[:TR] for i in range(0, len(echelon), TR)] or [[total] * TR]
    tiles.append([total] * TR)
    assert len(tiles) == DX.rref_tiles(n)
    V = np.concatenate([np.tile(np.array(t, dtype=np.uint64), (grid, 1)) for t in tiles] + [np.array([total] * 5, dtype=np.uint64)])
    assert V.shape == (DX.rref_rows(n, cus()), n)
    with blz.Context(p, n) as ctx:
        for pad in (0, 3):
            xv, xb = F.to_dev(V, pad)
            e, z, info = ctx.rref(xv)
            assert np.array_equal(info.cpu().numpy(), info_of(r, piv, n)), pad
            assert same(e, E) and same(z, Z), pad
            assert F.padding_intact(xb, n) and same(xv, V), pad
            assert not F.to_host(ctx.combine([(e, z)])).any(), pad                  # e * z = 0


# ------------------------------------------------------------------------------------------ E. the iteration, rebuilt


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", DX.ITER_CASES, ids=[case_id(p, n) for n, p in DX.ITER_CASES])
def test_one_rebuilt_iteration_per_new_class(n, p, right, monkeypatch):
    """six steps of apply_pair, dot_pair, ortho_coeffs and combine_pair in place, against blz_iterate on a twin"""
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    F.four_calls_against_twin(n, p, right, 6, deficient=False)
