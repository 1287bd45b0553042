"""Fused device calls on the GPU: blz_apply_pair_device (Context.apply_pair), blz_dot_pair_device (Context.dot_pair) and
blz_combine_pair_device (Context.combine_pair) on caller-owned torch tensors, against

  - Python-integer sums and the unfused calls they replace (two Context.dot, two Context.combine on copies, two Context.apply);
  - blz_iterate on a twin context: the iteration rebuilt from FOUR calls -- apply_pair, dot_pair, ortho_coeffs, combine_pair in
    place on v and p -- with nothing read on the host inside the loop, from the usual and from a rank-deficient start, and on
    past the stop;
  - an undisturbed twin for "the solve is left alone".

Every comparison is equality of u64 words.  The reducer ladder -- every reducer class of csrc/modp.h, the widths between
those of WIDTHS, sums past ModP::chunk in the paired k_dev_dot and k_dev_combine2 -- is tests/test_gpu_device_exact.py, which imports the
helpers, MASKS and four_calls_against_twin from here.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import blz
from test_gpu_device_algebra import one_base_two_strides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P2, P3, P16, P31 = 2, 3, 65537, (1 << 31) - 1
P61, P61B, P62 = (1 << 61) - 1, (1 << 61) - 31, (1 << 62) - 57
PRIMES = (P2, P3, P16, P31, P61, P61B, P62)
PIDS = ("p2", "p3", "p16", "p31", "p61", "p61b", "p62")
WIDTHS = (1, 3, 5, 8, 16, 64)
PADS = (0, 2, 3)                                        # strides n, n + 2 and n + 3: the 16-byte and the 8-byte lane forms
SENTINEL = 0xDEADBEEFCAFEF00D
DEV = "cuda:0"
ITER_CASES = ((8, P61), (3, P16), (16, P61B))           # the grid of test_the_iteration_rebuilt_with_nothing_on_the_host
ITER_IDS = ("n8p61", "n3p16", "n16p61b")
_R = {}


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


def obj(a):
    return np.asarray(a).astype(object)


def words(a):
    return np.array(a, dtype=np.uint64)


def flat(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def residues(rows, n, p, seed):
    """random residues with 0 and p - 1 planted in whole rows; made once, never changed"""
    key = (rows, n, p, seed)
    if key not in _R:
        rng = np.random.default_rng([seed, rows, n])
        w = rng.integers(0, p, size=(rows, n), dtype=np.uint64)
        if rows:
            w[rng.integers(0, rows, 3)] = 0
            w[rng.integers(0, rows, 3)] = p - 1
        w.setflags(write=False)
        _R[key] = w
    return _R[key]


def coefficient(n, p, seed):
    rng = np.random.default_rng([seed, n, 7])
    a = rng.integers(0, p, size=(n, n), dtype=np.uint64)
    a[rng.integers(0, n), rng.integers(0, n)] = 0
    a[rng.integers(0, n), rng.integers(0, n)] = p - 1
    return a


def to_dev(w, pad=0, fill=SENTINEL):
    """(view of shape (rows, n) with row stride n + pad, the base tensor) on the device"""
    w = np.ascontiguousarray(w, dtype=np.uint64)
    base = np.full((w.shape[0], w.shape[1] + pad), fill, dtype=np.uint64)
    base[:, :w.shape[1]] = w
    tb = torch.from_numpy(base.view(np.int64)).to(DEV)
    return tb[:, :w.shape[1]], tb


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def to_host(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def sentinel(*shape):
    return torch.from_numpy(np.full(shape, SENTINEL, dtype=np.uint64).view(np.int64)).to(DEV)


def padding_intact(base, n):
    return (to_host(base)[:, n:] == SENTINEL).all()


def gram_ref(X, Y, p, n):
    return words((obj(X).T @ obj(Y)) % p).reshape(n, n)


# ------------------------------------------------------------------------------------------ 1. dot_pair


def tile_rows(n):
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return 1024 >> lg


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_dot_pair_against_exact_integers_and_two_dots(p, n):
    TR = tile_rows(n)
    with blz.Context(p, n) as ctx:                      # no matrix: the rows are the caller's
        for rows in (0, 1, 2, TR - 1, TR, TR + 1, 1000):
            A, B, Y = residues(rows, n, p, 1), residues(rows, n, p, 2), residues(rows, n, p, 3)
            H = {"A": A, "B": B, "Y": Y}
            exact = {k: gram_ref(X, Y, p, n) for k, X in H.items()} if rows * n * n <= 300000 else None     # Python integers
            for pad in PADS:
                (a, ab), (b, bb), (y, yb) = to_dev(A, pad), to_dev(B, pad), to_dev(Y, pad)
                T = {"A": a, "B": b, "Y": y}
                two = {k: to_host(ctx.dot(t, y)) for k, t in T.items()}          # the calls dot_pair replaces
                if exact:
                    assert all(np.array_equal(two[k], exact[k]) for k in T), (rows, pad)
                # the five aliasing patterns: all distinct, x1 = y, x0 = y, x0 = x1, all the same
                for tag, k0, k1 in (("distinct", "A", "B"), ("x1 is y", "A", "Y"), ("x0 is y", "Y", "B"), ("x0 is x1", "A", "A"),
                                    ("all one", "Y", "Y")):
                    c = ctx.dot_pair(T[k0], T[k1], y)
                    assert c.dtype == torch.uint64 and tuple(c.shape) == (2, n, n) and c.is_contiguous() and c.is_cuda
                    got = to_host(c)
                    assert np.array_equal(got[0], two[k0]), (rows, pad, tag, 0)
                    assert np.array_equal(got[1], two[k1]), (rows, pad, tag, 1)
                    if rows == 0:
                        assert not got.any()
                    if tag == "all one":                # both triangles of a Gram panel
                        assert np.array_equal(got[0], got[0].T) and np.array_equal(got[0], got[1])
                out = sentinel(2, n, n)                 # the caller's out: every word written (zeros at rows = 0)
                assert ctx.dot_pair(a, b, y, out=out) is out
                assert np.array_equal(to_host(out)[0], two["A"]) and np.array_equal(to_host(out)[1], two["B"])
                for v, base, W in ((a, ab, A), (b, bb, B), (y, yb, Y)):      # the inputs and their padding as they were
                    assert padding_intact(base, n) and np.array_equal(to_host(v), W)
            # mixed strides: one block of each lane form
            c = to_host(ctx.dot_pair(to_dev(A, 3)[0], to_dev(B, 0)[0], to_dev(Y, 2)[0]))
            assert np.array_equal(c[0], two["A"]) and np.array_equal(c[1], two["B"]), (rows, "mixed")
        # a sixth aliasing pattern: x0 = y = (base, stride n) are one block, x1 = (the same base, stride 2n) is another
        if n in (3, 8) and p in (P16, P62):
            for rows in (37, 300):                      # one partial tile; several workgroups
                near, far, N, F = one_base_two_strides(rows, n, p)
                got = to_host(ctx.dot_pair(near, far, near))
                assert np.array_equal(got[0], gram_ref(N, N, p, n)), (rows, "one pointer, two strides", 0)     # Python integers
                assert np.array_equal(got[1], gram_ref(F, N, p, n)), (rows, "one pointer, two strides", 1)


@pytest.mark.parametrize("n", (1, 8, 64))
@pytest.mark.parametrize("p", (P61, P62, P16), ids=("p61", "p62", "p16"))
def test_dot_pair_where_the_sums_are_largest(p, n):
    """4097 rows of p - 1: every product is (p - 1)^2 = 1 mod p, the unreduced sums are as large as they get"""
    rows = 4097
    with blz.Context(p, n) as ctx:
        x = torch.full((rows, n), p - 1, dtype=torch.int64, device=DEV)
        y = torch.full((rows, n + 3), p - 1, dtype=torch.int64, device=DEV)[:, :n]
        z = torch.full((rows, n + 2), p - 1, dtype=torch.int64, device=DEV)[:, :n]
        want = np.full((2, n, n), rows % p, dtype=np.uint64)
        for x0, x1, yy in ((x, y, z), (x, z, z), (y, y, y), (z, z, x), (x, x, x)):
            assert np.array_equal(to_host(ctx.dot_pair(x0, x1, yy)), want)


# ------------------------------------------------------------------------------------------ 2. combine_pair


def combine_ref(blocks, coeffs, p, n):
    rows = blocks[0].shape[0]
    z = np.zeros((rows, n), dtype=object)
    for X, A in zip(blocks, coeffs):
        if A is not None:
            z = z + obj(X) @ obj(A)
    return words(z % p).reshape(rows, n)


# which outputs a term enters, per number of terms; the three-term one is the update of a Lanczos step
MASKS = {1: [((1, 1),)],
         2: [((1, 0), (0, 1)), ((1, 1), (0, 1))],
         3: [((1, 0), (1, 1), (1, 1))],
         4: [((1, 1), (0, 1), (1, 0), (1, 1)), ((1, 1), (1, 1), (1, 1), (1, 1))]}


def combine_pair_case(ctx, p, n, rows, masks, pads, exact=True):
    nterms = len(masks)
    Xs = [residues(rows, n, p, 10 + t) for t in range(nterms)]
    A0 = [coefficient(n, p, 20 + t) if m[0] else None for t, m in enumerate(masks)]
    A1 = [coefficient(n, p, 30 + t) if m[1] else None for t, m in enumerate(masks)]
    tag = (rows, masks, pads)

    def fresh():
        return [to_dev(X, pads[t % len(pads)]) for t, X in enumerate(Xs)]

    def terms_of(devs, kind=0):
        # the coefficients as tensors, numpy arrays or nested lists
        conv = lambda A, t: None if A is None else (up(A) if (t + kind) % 3 == 0 else A if (t + kind) % 3 == 1 else A.tolist())
        return [(devs[t][0], conv(A0[t], t), conv(A1[t], t)) for t in range(nterms)]

    # the unfused composition on copies
    devs = fresh()
    w0 = to_host(ctx.combine([(devs[t][0], A0[t]) for t in range(nterms) if A0[t] is not None]))
    w1 = to_host(ctx.combine([(devs[t][0], A1[t]) for t in range(nterms) if A1[t] is not None]))
    if exact:
        assert np.array_equal(w0, combine_ref(Xs, A0, p, n)) and np.array_equal(w1, combine_ref(Xs, A1, p, n)), tag
    # z0 and z1 fresh
    z0, z1 = ctx.combine_pair(terms_of(devs))
    assert z0.dtype == z1.dtype == torch.uint64 and tuple(z0.shape) == tuple(z1.shape) == (rows, n)
    assert np.array_equal(to_host(z0), w0) and np.array_equal(to_host(z1), w1), tag
    (o0, b0), (o1, b1) = to_dev(np.full((rows, n), SENTINEL, dtype=np.uint64), 3), to_dev(np.full((rows, n), SENTINEL, dtype=np.uint64), 2)
    got = ctx.combine_pair(terms_of(devs, 1), out=(o0, o1))                     # the caller's strided outputs
    assert got[0] is o0 and got[1] is o1
    assert np.array_equal(to_host(o0), w0) and np.array_equal(to_host(o1), w1), tag
    assert padding_intact(b0, n) and padding_intact(b1, n)
    for t in range(nterms):                             # the inputs and their padding as they were
        assert np.array_equal(to_host(devs[t][0]), Xs[t]) and padding_intact(devs[t][1], n)
    # z0 in place on the last term, z1 fresh
    devs = fresh()
    z1 = sentinel(rows, n)
    ctx.combine_pair(terms_of(devs, 2), out=(devs[-1][0], z1))
    assert np.array_equal(to_host(devs[-1][0]), w0) and np.array_equal(to_host(z1), w1), tag + ("z0 in place",)
    assert padding_intact(devs[-1][1], n)
    # z1 in place on the first term, z0 fresh
    devs = fresh()
    z0 = sentinel(rows, n)
    ctx.combine_pair(terms_of(devs), out=(z0, devs[0][0]))
    assert np.array_equal(to_host(z0), w0) and np.array_equal(to_host(devs[0][0]), w1), tag + ("z1 in place",)
    # both in place on different terms: the Lanczos pattern
    if nterms >= 2:
        devs = fresh()
        ctx.combine_pair(terms_of(devs, 1), out=(devs[-2][0], devs[-1][0]))
        assert np.array_equal(to_host(devs[-2][0]), w0) and np.array_equal(to_host(devs[-1][0]), w1), tag + ("both in place",)
        assert padding_intact(devs[-2][1], n) and padding_intact(devs[-1][1], n)
        for t in range(nterms - 2):
            assert np.array_equal(to_host(devs[t][0]), Xs[t])


@pytest.mark.parametrize("n", (1, 3, 5, 8, 16))
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine_pair_against_exact_integers_and_two_combines(p, n):
    with blz.Context(p, n) as ctx:
        for rows in (0, 1, 63, 257):
            for nterms in (1, 2, 3, 4):
                for k, masks in enumerate(MASKS[nterms]):
                    for pads in ((0,), (2,), (3,), (0, 3, 2, 1)):
                        if pads != (0, 3, 2, 1) and (rows, k) not in ((63, 0), (257, 0)):
                            continue                    # the uniform strides at two row counts, the mixed ones everywhere
                        combine_pair_case(ctx, p, n, rows, masks, pads)


@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine_pair_at_n64(p):
    """five present panels are the whole LDS of a CU (one workgroup of 1024 threads); eight do not fit, and the terms whose
    panels are left over read them from global memory -- in the same single pass, in place included"""
    with blz.Context(p, 64) as ctx:
        five = ((1, 0), (1, 1), (1, 1))
        eight = ((1, 1), (1, 1), (1, 1), (1, 1))
        six = ((1, 1), (1, 1), (0, 1), (1, 0))          # the third term fits after the first two, the fourth with it
        for masks in (five, eight, six):
            for pads in ((0,), (3, 2, 0, 1)):
                combine_pair_case(ctx, p, 64, 70, masks, pads, exact=(pads == (0,) and masks != six))


@pytest.mark.parametrize("n", (8, 64))
@pytest.mark.parametrize("p", (P61, P62, P16), ids=("p61", "p62", "p16"))
def test_combine_pair_with_words_p_minus_1_throughout(p, n):
    """every block word and every coefficient is p - 1: each product is 1 mod p, so an output word is n times its terms"""
    rows = 300
    with blz.Context(p, n) as ctx:
        full = torch.full((n, n), p - 1, dtype=torch.int64, device=DEV)
        xs = [torch.full((rows, n + pad), p - 1, dtype=torch.int64, device=DEV)[:, :n] for pad in (0, 3, 2, 0)]
        terms = [(xs[0], full, None), (xs[1], full, full), (xs[2], full, full), (xs[3], full, full)]
        z0, z1 = ctx.combine_pair(terms)
        assert (to_host(z0) == np.uint64(4 * n % p)).all() and (to_host(z1) == np.uint64(3 * n % p)).all()
        ctx.combine_pair(terms[:3], out=(xs[1], xs[2]))
        assert (to_host(xs[1]) == np.uint64(3 * n % p)).all() and (to_host(xs[2]) == np.uint64(2 * n % p)).all()


# ------------------------------------------------------------------------------------------ 3. apply_pair


def apply_pair_cases(make, p, n, seed=8):
    """apply_pair against two apply calls on a context made the same way: both orders, with and without the intermediate, into
    the caller's strided blocks, and in place"""
    with make() as ctx, make() as ref:
        for first in (False, True):
            xr, yr = ctx.apply_rows(first)
            assert ctx.apply_rows(not first) == (yr, xr)
            for kind in ("random", "max"):
                X = residues(xr, n, p, seed) if kind == "random" else np.full((xr, n), p - 1, dtype=np.uint64)
                mid_want = ref.apply(first, to_dev(X)[0])
                want = to_host(ref.apply(not first, mid_want))
                mid_want = to_host(mid_want)
                x, xb = to_dev(X, 3)
                z = ctx.apply_pair(first, x)
                assert z.dtype == torch.uint64 and tuple(z.shape) == (xr, n)
                assert np.array_equal(to_host(z), want), (first, kind)
                z, mid = ctx.apply_pair(first, x, mid=True)
                assert tuple(mid.shape) == (yr, n)
                assert np.array_equal(to_host(z), want) and np.array_equal(to_host(mid), mid_want), (first, kind, "mid")
                (out, ob), (m, mb) = to_dev(np.zeros((xr, n), dtype=np.uint64), 2), to_dev(np.zeros((yr, n), dtype=np.uint64), 3)
                got = ctx.apply_pair(first, x, out=out, mid=m)
                assert got[0] is out and got[1] is m
                assert np.array_equal(to_host(out), want) and np.array_equal(to_host(m), mid_want)
                assert padding_intact(ob, n) and padding_intact(mb, n) and padding_intact(xb, n)
                assert np.array_equal(to_host(x), X)
                assert ctx.apply_pair(first, x, out=x) is x                     # in place
                assert np.array_equal(to_host(x), want) and padding_intact(xb, n), (first, kind, "in place")
        assert ctx.iterations == 0


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("name, p, n", (("rand300x200", P61, 8), ("rand300x200", P16, 5), ("quirks40x30", P61B, 16),
                                         ("quirks40x30", P31, 3)), ids=("rand-p61n8", "rand-p16n5", "quirks-p61bn16", "quirks-p31n3"))
def test_apply_pair_against_two_applies(name, p, n, right):
    M = blz.Matrix.load(path(name), p)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix(M, right)
        return ctx
    apply_pair_cases(make, p, n)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
def test_apply_pair_in_signed_mode(right):
    p, n = P61, 8
    M = blz.Matrix.load_signed(path("graph200x600"))

    def make():
        ctx = blz.Context(p, n)
        ctx.set_values_signed()
        ctx.set_matrix(M, right)
        assert ctx.slab_signed(False) and ctx.slab_signed(True)
        return ctx
    apply_pair_cases(make, p, n)


@pytest.mark.parametrize("name", ("wide120x260", "rand3000x2000"))
@pytest.mark.parametrize("p", (P61, P61B), ids=("p61", "p61b"))
def test_apply_pair_in_wide_mode(p, name):
    n = 4
    base = blz.Matrix.load(path(name), p)
    hi = np.random.default_rng(12).integers(0, 1 << 28, base.nnz, dtype=np.uint32)     # entries up to 2^60: residues below p
    M = blz.Matrix(base.nrows, base.ncols, base.i, base.j, base.x, x_hi=hi)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix(M, True)
        assert ctx.values_wide() and ctx.slab_wide(False) and ctx.slab_wide(True)
        return ctx
    apply_pair_cases(make, p, n)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("k", (1, 3))
def test_apply_pair_on_a_bordered_context(k, right):
    p, n = P61, 4
    M = blz.Matrix.load(path("rand3000x2000"), p)
    b = residues(M.nrows if right else M.ncols, k, p, seed=k)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix_rhs_block(M, b, right)
        assert ctx.rhs_count == k
        return ctx
    apply_pair_cases(make, p, n)


# ------------------------------------------------------------------------------------------ 4. the iteration from four calls


def fused_step(ctx, right, v, pb):
    """sequential/lanczos_modp.c:635-656 in four calls, v and p updated in place: nothing is read on the host"""
    Av = ctx.apply_pair(not right, v)
    c = ctx.dot_pair(v, Av, Av)                         # vtAv, vtAAv
    coef, npiv = ctx.ortho_coeffs(c[0], c[1])
    ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))
    return c, coef, npiv


def deficient_start(v0, n):
    """column 1 <- column 0, column 2 <- 0 (nothing at n = 1)"""
    v0 = v0.copy()
    if n >= 2:
        v0[:, 1] = v0[:, 0]
    if n >= 3:
        v0[:, 2] = 0
    return v0


def four_calls_against_twin(n, p, right, steps, deficient):
    M = blz.Matrix.load(path("rand300x200"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M, right)                        # never iterates
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v0 = twin.get_block(blz.V).reshape(rows, n)
        if deficient:
            v0 = deficient_start(v0, n)
            twin.set_block(blz.V, v0.reshape(-1))
        want = []
        for _ in range(steps):
            done, stopped = twin.iterate(1)[:2]
            want.append((done, stopped, twin.get_small(blz.VTAV), twin.get_small(blz.VTAAV), twin.get_small(blz.D),
                         twin.get_block(blz.V), twin.get_block(blz.P)))
        v, pb = to_dev(v0)[0].contiguous(), torch.zeros((rows, n), dtype=torch.int64, device=DEV)
        got = []
        for _ in range(steps):                          # no tensor is read on the host in here
            c, coef, npiv = fused_step(ctx, right, v, pb)
            got.append((v.clone(), pb.clone(), c, coef, npiv))
        assert ctx.iterations == 0
        got = [tuple(to_host(t) for t in rec) for rec in got]
    for step, ((gv, gp, c, coef, npiv), (done, stopped, wA, wAA, wd, wv, wp)) in enumerate(zip(got, want)):
        assert (done, stopped) == (1, False), step
        assert np.array_equal(c[0].reshape(-1), wA) and np.array_equal(c[1].reshape(-1), wAA), step
        assert np.array_equal(np.diagonal(coef[blz.COEF_V_AV]), wd) and int(npiv[0]) == int(wd.sum()) > 0, step
        assert np.array_equal(gv.reshape(-1), wv), step
        assert np.array_equal(gp.reshape(-1), wp), step
    return got


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_the_iteration_rebuilt_from_four_calls(n, p, right, monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    four_calls_against_twin(n, p, right, 6, deficient=False)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_the_four_calls_from_a_rank_deficient_start(n, p, right, monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    got = four_calls_against_twin(n, p, right, 6, deficient=True)
    pattern = np.array([1, 0, 0] + [1] * (n - 3), dtype=np.uint64)
    for step, rec in enumerate(got):
        assert np.array_equal(np.diagonal(rec[3][blz.COEF_V_AV]), pattern) and int(rec[4][0]) == n - 2, step


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_twenty_steps_past_the_stop_change_nothing(n, p, right, monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    M = blz.Matrix.load(path("rand300x200"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M, right)
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v = to_dev(twin.get_block(blz.V).reshape(rows, n))[0].contiguous()
        pb = torch.zeros_like(v)
        done, stopped = twin.iterate(200)[:2]
        assert stopped and 0 < done < 80
        for _ in range(done + 1):                       # the step that finds npiv = 0 included
            _, _, npiv = fused_step(ctx, right, v, pb)
        at_stop = (v.clone(), pb.clone())
        for _ in range(20):
            _, _, npiv = fused_step(ctx, right, v, pb)
        assert int(to_host(npiv)[0]) == 0
        assert torch.equal(v, at_stop[0]) and torch.equal(pb, at_stop[1])
        assert np.array_equal(to_host(v).reshape(-1), twin.get_block(blz.V))
        assert np.array_equal(to_host(pb).reshape(-1), twin.get_block(blz.P))
        assert ctx.iterations == 0 and twin.iterations == done


# ------------------------------------------------------------------------------------------ 5. the solve is not disturbed


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(s, t) for s, t in zip(a, b))


def foreign_calls(ctx, ref, p, n):
    """the three calls on tensors that have nothing to do with the solve; all checked (ref: a context that only applies)"""
    X, Y, Z = residues(777, n, p, 51), residues(777, n, p, 52), residues(777, n, p, 53)
    A, B = coefficient(n, p, 54), coefficient(n, p, 55)
    x, y, z = to_dev(X, 3)[0], to_dev(Y)[0], to_dev(Z, 2)[0]
    c = to_host(ctx.dot_pair(x, y, y))
    assert np.array_equal(c[0], gram_ref(X, Y, p, n)) and np.array_equal(c[1], gram_ref(Y, Y, p, n))
    ctx.combine_pair([(x, A, None), (y, B, A), (z, A, B)], out=(y, z))
    assert np.array_equal(to_host(y), combine_ref([X, Y, Z], [A, B, A], p, n))
    assert np.array_equal(to_host(z), combine_ref([X, Y, Z], [None, A, B], p, n))
    xr, _ = ctx.apply_rows(False)
    W = residues(xr, n, p, 56)
    got, mid = ctx.apply_pair(False, to_dev(W)[0], mid=True)
    assert np.array_equal(to_host(mid), to_host(ref.apply(False, to_dev(W)[0])))
    assert np.array_equal(to_host(got), to_host(ref.apply(True, mid)))


def test_the_fused_calls_leave_the_solve_alone(monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")        # p implicit while the iteration runs
    p, n = P61, 8
    M = blz.Matrix.load(path("rand3000x2000"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin, blz.Context(p, n) as ref:
        ref.set_matrix(M)
        for c in (ctx, twin):
            c.set_matrix(M)
            c.init_v()
            assert c.iterate(3)[:2] == (3, False)
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        foreign_calls(ctx, ref, p, n)                   # while p is implicit: the flag and the count do not move
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        before = state(ctx)
        assert same(before, state(twin))
        foreign_calls(ctx, ref, p, n)
        assert same(before, state(ctx))
        stopped = False
        while not stopped:                              # on to the stop, the calls between the batches
            stopped = ctx.iterate(16)[1]
            assert twin.iterate(16)[1] == stopped
            foreign_calls(ctx, ref, p, n)
            assert np.array_equal(ctx.get_small(blz.VTAV), twin.get_small(blz.VTAV)) and ctx.iterations == twin.iterations
        assert ctx.iterations == twin.iterations > 3
        assert same(state(ctx), state(twin))
        assert ctx.final_check() == twin.final_check()
        foreign_calls(ctx, ref, p, n)
        assert same(state(ctx), state(twin))


# ------------------------------------------------------------------------------------------ 6. stream order


def test_the_calls_are_ordered_on_the_callers_stream():
    p, n, rows = P61, 8, 3000
    a, b, Y, Z = (residues(rows, n, p, 41 + k) for k in range(4))
    A, B = coefficient(n, p, 45), coefficient(n, p, 46)
    M = blz.Matrix.load(path("rand3000x2000"), p)
    x_host = words((obj(a) + obj(b)) % p)
    plus1 = lambda t: words((obj(t) + 1) % p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as ref:
        for c in (ctx, ref):
            c.set_matrix(M)
        assert ctx.apply_rows(False) == (2000, 3000)
        want_z = to_host(ref.apply(True, ref.apply(False, to_dev(x_host[:2000])[0])))
        ta, tb, ty, tz, tA, tB = up(a), up(b), up(Y), up(Z), up(A), up(B)
        ctx.dot_pair(ta, ty, ty)                        # (scratch, slabs and events are in place: nothing synchronous is left)
        ctx.apply_pair(False, ta[:2000].contiguous())
        big = torch.rand(2048, 2048, device=DEV)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            for _ in range(20):                         # a few milliseconds of work ahead of x on this stream
                big = torch.nn.functional.normalize(big @ big)
            x = torch.remainder(ta + tb + (big[0, 0] > 2).to(torch.int64), p)      # (a + b) mod p, behind the products above
            c = ctx.dot_pair(x, ty, ty)                 # stream=None: torch's current stream, which is s
            z0, z1 = ctx.combine_pair([(x, tA, tB), (ty, tB, None), (tz, None, tA)])
            w = ctx.apply_pair(False, x[:2000])
            used = [torch.remainder(t.view(torch.int64) + 1, p) for t in (c, z0, z1, w)]      # consumed at once
            got = [t.cpu().numpy().view(np.uint64) for t in used]
    assert np.array_equal(got[0][0], plus1(gram_ref(x_host, Y, p, n))) and np.array_equal(got[0][1], plus1(gram_ref(Y, Y, p, n)))
    assert np.array_equal(got[1], plus1(combine_ref([x_host, Y, Z], [A, B, None], p, n)))
    assert np.array_equal(got[2], plus1(combine_ref([x_host, Y, Z], [B, None, A], p, n)))
    assert np.array_equal(got[3], plus1(want_z))


# ------------------------------------------------------------------------------------------ 7. refusals


def raw_apply2(ctx, x, ldx, y, ldy, z, ldz, first=0, stream=None):
    return blz.lib().blz_apply_pair_device(ctx.h, C.c_int(first), C.c_void_p(x), C.c_int64(ldx), C.c_void_p(y), C.c_int64(ldy),
                                           C.c_void_p(z), C.c_int64(ldz), stream)


def raw_dot2(ctx, rows, x0, ld0, x1, ld1, y, ldy, c, stream=None):
    return blz.lib().blz_dot_pair_device(ctx.h, C.c_int64(rows), C.c_void_p(x0), C.c_int64(ld0), C.c_void_p(x1), C.c_int64(ld1),
                                         C.c_void_p(y), C.c_int64(ldy), C.c_void_p(c), stream)


def raw_combine2(ctx, rows, xs, lds, a0, a1, z0, ldz0, z1, ldz1, nterms=None, stream=None):
    k = len(xs)
    return blz.lib().blz_combine_pair_device(ctx.h, C.c_int64(rows), C.c_int(k if nterms is None else nterms), (C.c_void_p * k)(*xs),
                                             (C.c_int64 * k)(*lds), (C.c_void_p * k)(*a0), (C.c_void_p * k)(*a1), C.c_void_p(z0),
                                             C.c_int64(ldz0), C.c_void_p(z1), C.c_int64(ldz1), stream)


def refused(rc, *parts):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL, (rc, msg)
    for w in parts:
        assert w in msg, msg
    return msg


def test_refusals_launch_nothing(monkeypatch):
    p, n, rows = P61, 8, 114
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    M = blz.Matrix.synth(rows, rows, 4 * rows, 5, p)    # square: x, y and z of apply_pair have `rows` rows
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        assert ctx.apply_rows(False) == (rows, rows)
        x, y = up(residues(rows, n, p, 61)), up(residues(rows, n, p, 62))
        a = up(coefficient(n, p, 63))
        x0, y0, a0 = to_host(x).copy(), to_host(y).copy(), to_host(a).copy()
        c, z, w, both = sentinel(2, n, n), sentinel(rows, n), sentinel(rows, n), sentinel(2 * rows, n)
        X, Y, A, Cc, Z, W, Bp = (t.data_ptr() for t in (x, y, a, c, z, w, both))
        ok = [sentinel(rows, n) for _ in range(3)]      # (the calls below are well formed but for one thing)
        assert raw_dot2(ctx, rows, X, n, Y, n, Y, n, sentinel(2, n, n).data_ptr()) == blz.OK
        assert raw_combine2(ctx, rows, [X, Y], [n, n], [A, 0], [A, A], ok[0].data_ptr(), n, ok[1].data_ptr(), n) == blz.OK
        assert raw_apply2(ctx, X, n, ok[0].data_ptr(), n, ok[1].data_ptr(), n) == blz.OK
        assert raw_apply2(ctx, X, n, 0, 0, ok[1].data_ptr(), n) == blz.OK                      # y may be NULL, ldy is ignored
        assert raw_dot2(ctx, 0, 0, n, 0, n, 0, n, sentinel(2, n, n).data_ptr()) == blz.OK      # no rows: any block pointer
        assert raw_combine2(ctx, 0, [0], [n], [A], [A], 0, n, 0, n) == blz.OK
        # a host address for each argument in turn
        hb, hs = np.zeros((rows, n), dtype=np.uint64), np.zeros((2, n, n), dtype=np.uint64)
        H, HS = hb.ctypes.data, hs.ctypes.data
        refused(raw_dot2(ctx, rows, H, n, Y, n, Y, n, Cc), " x0 ", "not device memory")
        refused(raw_dot2(ctx, rows, X, n, H, n, Y, n, Cc), " x1 ", "not device memory")
        refused(raw_dot2(ctx, rows, X, n, Y, n, H, n, Cc), " y ", "not device memory")
        refused(raw_dot2(ctx, rows, X, n, Y, n, Y, n, HS), " c ", "not device memory")
        refused(raw_combine2(ctx, rows, [X, H], [n, n], [A, A], [A, A], Z, n, W, n), "x[1]", "not device memory")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [HS, A], [A, A], Z, n, W, n), "a0[0]", "not device memory")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, HS], Z, n, W, n), "a1[1]", "not device memory")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], H, n, W, n), " z0 ", "not device memory")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, H, n), " z1 ", "not device memory")
        refused(raw_apply2(ctx, H, n, Z, n, W, n), " x ", "not device memory")
        refused(raw_apply2(ctx, X, n, H, n, W, n), " y ", "not device memory")
        refused(raw_apply2(ctx, X, n, Z, n, H, n), " z ", "not device memory")
        # a NULL entry
        refused(raw_dot2(ctx, rows, 0, n, Y, n, Y, n, Cc), "x0 is NULL")
        refused(raw_dot2(ctx, rows, X, n, Y, n, Y, n, 0), "c is NULL")
        refused(raw_combine2(ctx, rows, [X, 0], [n, n], [A, A], [A, A], Z, n, W, n), "x[1] is NULL")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], 0, n, W, n), "z0 is NULL")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, 0, n), "z1 is NULL")
        refused(raw_apply2(ctx, 0, n, Z, n, W, n), "x is NULL")
        refused(raw_apply2(ctx, X, n, Z, n, 0, n), "z is NULL")
        # one word short: 114 rows at a stride of 9 words are 1025 words; the allocation has 1024
        ld = 9
        assert ((rows - 1) * ld + n) * 8 == 8192 + 8
        short, sq, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for hnd, size in ((short, 8192), (sq, n * n * 8 - 8), (pr, 2 * n * n * 8 - 8)):
            assert hip.hipMalloc(C.byref(hnd), C.c_size_t(size)) == 0
        try:
            refused(raw_dot2(ctx, rows, short.value, ld, Y, n, Y, n, Cc), " x0 ", "allocation ends")
            refused(raw_dot2(ctx, rows, X, n, short.value, ld, Y, n, Cc), " x1 ", "allocation ends")
            refused(raw_dot2(ctx, rows, X, n, Y, n, short.value, ld, Cc), " y ", "allocation ends")
            refused(raw_dot2(ctx, rows, X, n, Y, n, Y, n, pr.value), " c ", "allocation ends")
            refused(raw_combine2(ctx, rows, [X, short.value], [n, ld], [A, A], [A, A], Z, n, W, n), "x[1]", "allocation ends")
            refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, sq.value], [A, A], Z, n, W, n), "a0[1]", "allocation ends")
            refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [sq.value, A], Z, n, W, n), "a1[0]", "allocation ends")
            refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], short.value, ld, W, n), " z0 ", "allocation ends")
            refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, short.value, ld), " z1 ", "allocation ends")
            refused(raw_apply2(ctx, short.value, ld, Z, n, W, n), " x ", "allocation ends")
            refused(raw_apply2(ctx, X, n, short.value, ld, W, n), " y ", "allocation ends")
            refused(raw_apply2(ctx, X, n, Z, n, short.value, ld), " z ", "allocation ends")
        finally:
            torch.cuda.synchronize()
            for hnd in (short, sq, pr):
                assert hip.hipFree(hnd) == 0
        # ld < n
        refused(raw_dot2(ctx, rows, X, n - 1, Y, n, Y, n, Cc), " x0 ", "less than n")
        refused(raw_dot2(ctx, rows, X, n, Y, 0, Y, n, Cc), " x1 ", "less than n")
        refused(raw_dot2(ctx, rows, X, n, Y, n, Y, n - 1, Cc), " y ", "less than n")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n - 1], [A, A], [A, A], Z, n, W, n), "x[1]", "less than n")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n - 1, W, n), " z0 ", "less than n")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, W, 0), " z1 ", "less than n")
        refused(raw_apply2(ctx, X, n - 1, Z, n, W, n), " x ", "less than n")
        refused(raw_apply2(ctx, X, n, Z, n - 1, W, n), " y ", "less than n")
        refused(raw_apply2(ctx, X, n, Z, n, W, n - 1), " z ", "less than n")
        with pytest.raises(ValueError):
            ctx.dot_pair(x[:, :n - 1], y, y)
        # the number of terms, the number of rows
        refused(raw_combine2(ctx, rows, [X], [n], [A], [A], Z, n, W, n, nterms=0), "nterms = 0")
        refused(raw_combine2(ctx, rows, [X] * 5, [n] * 5, [A] * 5, [A] * 5, Z, n, W, n), "nterms = 5")
        refused(raw_dot2(ctx, -1, X, n, Y, n, Y, n, Cc), "rows = -1")
        refused(raw_combine2(ctx, -1, [X], [n], [A], [A], Z, n, W, n), "rows = -1")
        for bad in ([], [(x, a, a)] * 5):
            with pytest.raises(ValueError):
                ctx.combine_pair(bad)
        # a term absent from both outputs, an output with no term
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, 0], [A, 0], Z, n, W, n), "term 1", "neither output")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [0, 0], Z, n, W, n), "output z1", "no term")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [0, 0], [A, A], Z, n, W, n), "output z0", "no term")
        with pytest.raises(ValueError):
            ctx.combine_pair([(x, a, a), (y, None, None)], out=(z, w))
        with pytest.raises(ValueError):
            ctx.combine_pair([(x, a, None), (y, a, None)], out=(z, w))
        # every forbidden overlap
        half = rows // 2
        refused(raw_dot2(ctx, rows, Bp, n, Y, n, Y, n, Bp + 8 * n * (rows - 1)), "c overlaps x0")
        refused(raw_dot2(ctx, rows, X, n, Bp, n, Y, n, Bp), "c overlaps x1")
        refused(raw_dot2(ctx, rows, X, n, Y, n, Bp, n, Bp + 8), "c overlaps y")
        refused(raw_combine2(ctx, rows, [Bp, Y], [n, n], [A, A], [A, A], Bp + 8 * n, n, W, n), "z0 overlaps x[0]")      # a row on
        refused(raw_combine2(ctx, half, [X, Bp], [n, n], [A, A], [A, A], Z, n, Bp, 2 * n), "z1 overlaps x[1]")          # another stride
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Bp, n, Bp + 8 * n * (rows - 1), n), "z0 overlaps z1")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], X, n, X, n), "z0 overlaps z1")                  # both ON one term
        refused(raw_combine2(ctx, n, [X, Y], [n, n], [A, Bp + 8], [A, A], Bp, n, W, n), "z0 overlaps a0[1]")
        refused(raw_combine2(ctx, n, [X, Y], [n, n], [A, A], [Bp, A], Bp, n, W, n), "z0 overlaps a1[0]")
        refused(raw_combine2(ctx, n, [X, Y], [n, n], [Bp, A], [A, A], Z, n, Bp, n), "z1 overlaps a0[0]")
        refused(raw_combine2(ctx, n, [X, Y], [n, n], [A, A], [A, Bp + 8], Z, n, Bp, n), "z1 overlaps a1[1]")
        refused(raw_apply2(ctx, Bp, n, 0, 0, Bp + 8 * n, n), "z overlaps x")                   # a row on: not the in-place form
        refused(raw_apply2(ctx, Bp, n, 0, 0, Bp, n + 1), "z overlaps x")                        # the pointer, another stride
        refused(raw_apply2(ctx, Bp, n, Bp + 8 * n * (rows - 1), n, W, n), "y overlaps x")
        refused(raw_apply2(ctx, X, n, Bp + 8 * n * (rows - 1), n, Bp, n), "y overlaps z")
        refused(raw_apply2(ctx, Bp, n, Bp, n, Bp, n), "y overlaps x")                           # in place, but y on top of it
        # a capturing stream
        s = torch.cuda.Stream(device=DEV)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rcs, msgs = [], []
            for call in (lambda: raw_dot2(ctx, rows, X, n, Y, n, Y, n, Cc, h),
                         lambda: raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, W, n, stream=h),
                         lambda: raw_apply2(ctx, X, n, Z, n, W, n, stream=h)):
                rcs.append(call())
                msgs.append(blz.lib().blz_last_error().decode())
            x.add_(0)                                   # (a graph of one node, not an empty one)
        assert rcs == [blz.EINVAL] * 3 and all("capturing" in m for m in msgs), (rcs, msgs)
        # nothing above ran: the outputs hold the sentinel, the inputs are what they were
        torch.cuda.synchronize()
        for t in (c, z, w, both):
            assert (to_host(t) == np.uint64(SENTINEL)).all()
        assert np.array_equal(to_host(x), x0) and np.array_equal(to_host(y), y0) and np.array_equal(to_host(a), a0)
    with blz.Context(p, n) as bare:                     # apply_pair needs a matrix; the other two do not
        rc = raw_apply2(bare, X, n, 0, 0, Z, n)
        assert rc == blz.EINVAL and "no matrix" in blz.lib().blz_last_error().decode()
    # a context with the collectives forced on
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")           # read when the communicator is attached
    one = blz.LoopGroup(1)
    ctx = blz.Context(p, n)
    try:
        ctx.comm_init_loopback(one, 0)
        for call in (lambda: ctx.dot_pair(x, y, y, out=c), lambda: ctx.combine_pair([(x, a, a)], out=(z, w))):
            with pytest.raises(blz.BlzError) as err:
                call()
            assert err.value.code == blz.EINVAL and "single rank" in str(err.value) and "BLZ_FORCE_COMM" in str(err.value)
        refused(raw_apply2(ctx, X, n, 0, 0, Z, n), "single rank", "BLZ_FORCE_COMM")
    finally:
        ctx.close()
        one.close()
    torch.cuda.synchronize()
    for t in (c, z, w):
        assert (to_host(t) == np.uint64(SENTINEL)).all()


def test_several_ranks_are_refused():
    p, n = P61, 4
    t = torch.zeros((100, n), dtype=torch.int64, device=DEV)
    a, c, z, w = sentinel(n, n), sentinel(2, n, n), sentinel(100, n), sentinel(100, n)
    grp = blz.LoopGroup(2)
    ctxs = [blz.Context(p, n) for _ in range(2)]
    try:
        for r, cx in enumerate(ctxs):
            cx.comm_init_loopback(grp, r)
        for cx in ctxs:
            refused(raw_dot2(cx, 100, t.data_ptr(), n, t.data_ptr(), n, t.data_ptr(), n, c.data_ptr()), "single rank")
            refused(raw_combine2(cx, 100, [t.data_ptr()], [n], [a.data_ptr()], [a.data_ptr()], z.data_ptr(), n, w.data_ptr(), n),
                    "single rank")
            refused(raw_apply2(cx, t.data_ptr(), n, 0, 0, z.data_ptr(), n), "single rank")
    finally:
        for cx in ctxs:
            cx.close()
        grp.close()
    torch.cuda.synchronize()
    for s in (c, z, w):
        assert (to_host(s) == np.uint64(SENTINEL)).all()
