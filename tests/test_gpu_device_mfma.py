"""Device block algebra on the matrix cores (csrc/blz_devmfma.hip): Context.dot, dot_pair, combine and combine_pair at
p = 2^61 - 1, n = 8 and 16, with BLZ_DEV_MFMA_MIN_ROWS=0 so that every row count takes the matrix-core form.

Every case first asks Context.devalg_plan which form the call WILL take (1: matrix cores), then compares u64 words for
equality with an exact expectation -- recombinations: devmfma_ref.combine_exact on one period of rows, tiled (the update is
row-local); inner products: the closed forms mfma_digits_ref.const_dot / cycle_dot -- and then runs the same call on a context
created under BLZ_NO_MFMA=1 (plan: form 0) against the SAME expectation: if both forms miss, the expectation is what is wrong.
The inputs are chosen by their bytes (mfma_digits_ref.PATTERNS), the worst (block word, coefficient) pairs are the ones
tests/test_devmfma_ref.py finds.

    A. combine      B. combine_pair      C. dot and dot_pair      D. past the fold      E. fallbacks
    F. whole iterations against blz_iterate                       G. two loopback ranks
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import blz
import devmfma_ref as D
import mfma_digits_ref as R
import test_gpu_device_fused as F
import test_gpu_device_ranks as K
from device_exact import P57
from test_devmfma_ref import COMBINE_HIGHEST, COMBINE_LOWEST

pytestmark = pytest.mark.gpu

P61 = F.P61
DEV = F.DEV
ROWS = (1, 16, 17, 257, 4099)           # one row, one 16-row tile, a tile and a row, several wavefronts, several workgroups
PADS = (0, 2)                           # strides n and n + 2 (both even: the 16-byte lane accesses)
DOT_ROWS = (1, 63, 64, 65, 4097)        # around the 64-row tile the plan reports, and past one workgroup's four tiles


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def two_forms(n, p=P61):
    """(context with the matrix-core forms on at every row count, context created under BLZ_NO_MFMA=1)"""
    with contextlib.ExitStack() as st:
        with environment(BLZ_DEV_MFMA_MIN_ROWS="0", BLZ_NO_MFMA=None):
            on = st.enter_context(blz.Context(p, n))
        with environment(BLZ_DEV_MFMA_MIN_ROWS="0", BLZ_NO_MFMA="1"):
            off = st.enter_context(blz.Context(p, n))
        yield (on, 1), (off, 0)


def mat(a, n):
    return np.array(a, dtype=np.uint64).reshape(n, n)


def combine_inputs(n, nterms, kind):
    """(one period of every block as flat lists, coefficient lists) of a coefficient kind"""
    if kind in ("highest", "lowest"):
        bw, cw = COMBINE_HIGHEST if kind == "highest" else COMBINE_LOWEST
        return [[R.word(bw)] * n for _ in range(nterms)], [R.coef_const(R.word(cw), n) for _ in range(nterms)]
    per = [[w for row in R.cycle_period(n, 5 * t + 1) for w in row] for t in range(nterms)]    # another shift per term
    if kind == "const":
        return per, [R.coef_const(R.word("top_80"), n) for _ in range(nterms)]
    if kind == "cycle":
        return per, [R.coef_cycle(n, 3 * t) for t in range(nterms)]
    return per, [R.coef_rotation(n) for _ in range(nterms)]


KINDS = ("const", "cycle", "rotation", "highest", "lowest")


# ------------------------------------------------------------------------------------------ A. combine


@pytest.mark.parametrize("nterms", (1, 2, 3, 4))
@pytest.mark.parametrize("n", (8, 16))
def test_combine_on_the_matrix_cores(n, nterms):
    with two_forms(n) as forms:
        for kind in KINDS:
            per, coef = combine_inputs(n, nterms, kind)
            prows = len(per[0]) // n
            want_per = D.combine_exact(per, coef, prows, n)
            A = [mat(a, n) for a in coef]
            for rows in ROWS:
                Xs = [D.tiled(x, rows, n) for x in per]
                want = D.tiled(want_per, rows, n)
                for pad in PADS:
                    for ctx, form in forms:
                        tag = (kind, rows, pad, form)
                        assert ctx.devalg_plan(blz.DEVOP_COMBINE, rows, nterms)["form"] == form, tag
                        devs = [F.to_dev(X, pad) for X in Xs]
                        z = ctx.combine([(devs[t][0], A[t]) for t in range(nterms)])                # out of place
                        assert np.array_equal(F.to_host(z), want), tag
                        (o, ob) = F.to_dev(np.full((rows, n), F.SENTINEL, dtype=np.uint64), pad)    # the caller's strided z
                        ctx.combine([(devs[t][0], A[t]) for t in range(nterms)], out=o)
                        assert np.array_equal(F.to_host(o), want) and F.padding_intact(ob, n), tag
                        for t in range(nterms):
                            assert np.array_equal(F.to_host(devs[t][0]), Xs[t]) and F.padding_intact(devs[t][1], n), tag
                        for t in range(nterms):                                                     # in place on each term
                            devs = [F.to_dev(X, pad) for X in Xs]
                            ctx.combine([(devs[q][0], A[q]) for q in range(nterms)], out=devs[t][0])
                            assert np.array_equal(F.to_host(devs[t][0]), want), tag + ("in place", t)
                            assert all(F.padding_intact(b, n) for _, b in devs), tag
                            assert all(np.array_equal(F.to_host(devs[q][0]), Xs[q]) for q in range(nterms) if q != t), tag


# ------------------------------------------------------------------------------------------ B. combine_pair


def pair_cases(n):
    """(name, masks, (index of the term z0 is written on or None, the same for z1))"""
    cases = [("lanczos in place", ((1, 0), (1, 1), (1, 1)), (1, 2)),         # terms Av, v, p; z0 = v, z1 = p
             ("a0 is NULL", ((0, 1), (1, 1)), (None, None)),
             ("z0 in place, z1 fresh", ((1, 1), (1, 0), (0, 1)), (0, None))]
    if n == 16:
        cases.append(("four terms, every panel", ((1, 1), (1, 1), (1, 1), (1, 1)), (None, 3)))     # the largest image
    return cases


@pytest.mark.parametrize("n", (8, 16))
def test_combine_pair_on_the_matrix_cores(n):
    with two_forms(n) as forms:
        for name, masks, (ip0, ip1) in pair_cases(n):
            nterms = len(masks)
            for kind in ("cycle", "rotation", "lowest"):
                per, coef = combine_inputs(n, nterms, kind)
                coef1 = [R.coef_cycle(n, 7 + t) for t in range(nterms)]
                a0 = [coef[t] if m[0] else None for t, m in enumerate(masks)]
                a1 = [coef1[t] if m[1] else None for t, m in enumerate(masks)]
                prows = len(per[0]) // n
                w0_per, w1_per = D.combine_exact(per, a0, prows, n), D.combine_exact(per, a1, prows, n)
                A0 = [None if a is None else mat(a, n) for a in a0]
                A1 = [None if a is None else mat(a, n) for a in a1]
                for rows in ROWS:
                    Xs = [D.tiled(x, rows, n) for x in per]
                    w0, w1 = D.tiled(w0_per, rows, n), D.tiled(w1_per, rows, n)
                    for pad in PADS:
                        for ctx, form in forms:
                            tag = (name, kind, rows, pad, form)
                            assert ctx.devalg_plan(blz.DEVOP_COMBINE_PAIR, rows, nterms)["form"] == form, tag
                            devs = [F.to_dev(X, pad) for X in Xs]
                            z0 = devs[ip0][0] if ip0 is not None else F.to_dev(np.full((rows, n), F.SENTINEL, dtype=np.uint64), pad)[0]
                            z1 = devs[ip1][0] if ip1 is not None else F.to_dev(np.full((rows, n), F.SENTINEL, dtype=np.uint64), pad)[0]
                            got = ctx.combine_pair([(devs[t][0], A0[t], A1[t]) for t in range(nterms)], out=(z0, z1))
                            assert got[0] is z0 and got[1] is z1
                            assert np.array_equal(F.to_host(z0), w0) and np.array_equal(F.to_host(z1), w1), tag
                            assert all(F.padding_intact(b, n) for _, b in devs), tag
                            assert all(np.array_equal(F.to_host(devs[t][0]), Xs[t]) for t in range(nterms) if t not in (ip0, ip1)), tag


# ------------------------------------------------------------------------------------------ C. dot and dot_pair


CONST_PAIRS = (R.DOT_HIGHEST, R.DOT_LOWEST, R.DOT_LOWEST[::-1])
CYCLE_PAIRS = ((2, 9), (0, 0))


@pytest.mark.parametrize("n", (8, 16))
def test_dot_and_dot_pair_on_the_matrix_cores(n):
    with two_forms(n) as forms:
        for rows in DOT_ROWS:
            cases = []
            for an, bn in CONST_PAIRS:
                a, b = R.word(an), R.word(bn)
                cases.append(((an, bn), R.const_block(a, rows, n), R.const_block(b, rows, n), R.const_dot(a, b, rows, n)))
            for sv, sa in CYCLE_PAIRS:
                cases.append(((sv, sa), R.cycle_block(rows, n, sv), R.cycle_block(rows, n, sa), R.cycle_dot(rows, n, sv, sa)))
            for name, V, AV, (vtav, vtaav) in cases:
                vtav, vtaav = mat(vtav, n), mat(vtaav, n)
                for pad in PADS:
                    for ctx, form in forms:
                        tag = (name, rows, pad, form)
                        assert ctx.devalg_plan(blz.DEVOP_DOT, rows)["form"] == form, tag
                        assert ctx.devalg_plan(blz.DEVOP_DOT_PAIR, rows)["form"] == form, tag
                        if form == 1:
                            assert ctx.devalg_plan(blz.DEVOP_DOT, rows)["tile_rows"] == 64
                        (v, vb), (av, avb) = F.to_dev(V.reshape(rows, n), pad), F.to_dev(AV.reshape(rows, n), pad)
                        assert np.array_equal(F.to_host(ctx.dot(v, av)), vtav), tag
                        assert np.array_equal(F.to_host(ctx.dot(av, av)), vtaav), tag + ("gram",)      # x is y
                        c = F.to_host(ctx.dot_pair(v, av, av))                                          # x1 is y
                        assert np.array_equal(c[0], vtav) and np.array_equal(c[1], vtaav), tag
                        out = F.sentinel(2, n, n)                                   # the caller's out: every word written
                        assert ctx.dot_pair(v, av, av, out=out) is out
                        assert np.array_equal(F.to_host(out)[0], vtav) and np.array_equal(F.to_host(out)[1], vtaav), tag
                        out1 = F.sentinel(n, n)
                        assert ctx.dot(v, av, out=out1) is out1 and np.array_equal(F.to_host(out1), vtav), tag
                        assert F.padding_intact(vb, n) and F.padding_intact(avb, n)


@pytest.mark.parametrize("n", (8, 16))
def test_the_five_aliasing_patterns_of_dot_pair(n):
    shifts = {"A": 2, "B": 9, "Y": 4}
    with two_forms(n) as forms:
        for rows in (65, 4097):
            H = {k: R.cycle_block(rows, n, s).reshape(rows, n) for k, s in shifts.items()}
            want = {k: mat(R.cycle_dot(rows, n, s, shifts["Y"])[0], n) for k, s in shifts.items()}
            for ctx, form in forms:
                assert ctx.devalg_plan(blz.DEVOP_DOT_PAIR, rows)["form"] == form
                T = {k: F.to_dev(w, 2 if k == "B" else 0)[0] for k, w in H.items()}
                for tag, k0, k1 in (("distinct", "A", "B"), ("x1 is y", "A", "Y"), ("x0 is y", "Y", "B"), ("x0 is x1", "A", "A"),
                                    ("all one", "Y", "Y")):
                    got = F.to_host(ctx.dot_pair(T[k0], T[k1], T["Y"]))
                    assert np.array_equal(got[0], want[k0]) and np.array_equal(got[1], want[k1]), (rows, tag, form)


# ------------------------------------------------------------------------------------------ D. past the fold


def device_cycle(rows, n, shift):
    one = torch.from_numpy(np.array(R.cycle_period(n, shift), dtype=np.uint64).view(np.int64)).to(DEV)
    return one.repeat(rows // R.L + 1, 1)[:rows]


@pytest.mark.parametrize("n", (8, 16))
def test_dot_pair_past_the_fold_on_the_matrix_cores(n):
    """every wavefront folds its accumulators once and goes on: rows = tile_rows (fold_tiles + 1) wavefronts + 1, all three
    numbers from the plan"""
    with two_forms(n) as ((on, _), (off, _)):
        plan = on.devalg_plan(blz.DEVOP_DOT_PAIR, 1 << 40)
        assert plan["form"] == 1 and plan["fold_tiles"] > 0
        rows = plan["tile_rows"] * (plan["fold_tiles"] + 1) * plan["wavefronts"] + 1
        assert on.devalg_plan(blz.DEVOP_DOT_PAIR, rows)["wavefronts"] == plan["wavefronts"]
        assert 3 * rows * n * 8 <= 4.5e9, "three blocks of this many rows must stay allocatable"
        cases = [("const", R.DOT_HIGHEST)]
        if n == 8:
            cases += [("const", R.DOT_LOWEST), ("cycle", (2, 9))]
        for kind, pair in cases:
            if kind == "const":
                a, b = R.word(pair[0]), R.word(pair[1])
                v = torch.full((rows, n), a, dtype=torch.int64, device=DEV)
                av = torch.full((rows, n), b, dtype=torch.int64, device=DEV)
                vtav, vtaav = R.const_dot(a, b, rows, n)
            else:
                v, av = device_cycle(rows, n, pair[0]), device_cycle(rows, n, pair[1])
                vtav, vtaav = R.cycle_dot(rows, n, *pair)
            for ctx, form in ((on, 1), (off, 0)):
                assert ctx.devalg_plan(blz.DEVOP_DOT_PAIR, rows)["form"] == form
                c = F.to_host(ctx.dot_pair(v, av, av))
                assert np.array_equal(c[0], mat(vtav, n)) and np.array_equal(c[1], mat(vtaav, n)), (kind, pair, form)
            del v, av


# ------------------------------------------------------------------------------------------ E. fallbacks


def offset_view(w):
    """the block in a tensor whose base is one word past a 16-byte boundary"""
    rows, n = w.shape
    flat = torch.zeros(rows * n + 1, dtype=torch.int64, device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(rows, n)
    v.copy_(torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(DEV))
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("n", (8, 16))
def test_blocks_that_are_not_16_byte_aligned_take_the_vector_form(n):
    rows = 257
    per, coef = combine_inputs(n, 2, "cycle")
    Xs = [D.tiled(x, rows, n) for x in per]
    want = D.tiled(D.combine_exact(per, coef, len(per[0]) // n, n), rows, n)
    A = [mat(a, n) for a in coef]
    vtav, vtaav = (mat(w, n) for w in R.cycle_dot(rows, n, 1, 6))       # the shifts of combine_inputs' two blocks
    with two_forms(n) as ((on, _), _):
        for op in (blz.DEVOP_DOT, blz.DEVOP_DOT_PAIR, blz.DEVOP_COMBINE, blz.DEVOP_COMBINE_PAIR):
            assert on.devalg_plan(op, rows, 2, aligned=True)["form"] == 1
            assert on.devalg_plan(op, rows, 2, aligned=False)["form"] == 0
        for make in (offset_view, lambda w: F.to_dev(w, 1)[0]):         # base off by one word; ld = n + 1
            x0, x1 = make(Xs[0]), make(Xs[1])
            assert np.array_equal(F.to_host(on.combine([(x0, A[0]), (x1, A[1])])), want)
            z0, z1 = on.combine_pair([(x0, A[0], None), (x1, A[1], A[1])])
            assert np.array_equal(F.to_host(z0), want)
            assert np.array_equal(F.to_host(on.dot(x0, x1)), vtav)
            c = F.to_host(on.dot_pair(x0, x1, x1))
            assert np.array_equal(c[0], vtav) and np.array_equal(c[1], vtaav)
            # one block of the call is enough
            aligned = F.to_dev(Xs[0], 0)[0]
            assert np.array_equal(F.to_host(on.combine([(aligned, A[0]), (x1, A[1])])), want)
            assert np.array_equal(F.to_host(on.dot(aligned, x1)), vtav)


def test_other_primes_widths_and_small_calls_take_the_vector_form():
    ops = (blz.DEVOP_DOT, blz.DEVOP_DOT_PAIR, blz.DEVOP_COMBINE, blz.DEVOP_COMBINE_PAIR)
    with environment(BLZ_DEV_MFMA_MIN_ROWS="0", BLZ_NO_MFMA=None):
        with blz.Context(P57, 8) as c57, blz.Context(P61, 4) as c4, blz.Context(P61, 8) as c8:
            for op in ops:
                assert c57.devalg_plan(op, 100000)["form"] == 0 and c4.devalg_plan(op, 100000)["form"] == 0
                assert c8.devalg_plan(op, 100000)["form"] == 1 and c8.devalg_plan(op, 100000)["min_rows"] == 0
                assert c8.devalg_plan(op, 0)["form"] == 0           # no rows: nothing to multiply
            with pytest.raises(blz.BlzError) as e:
                c8.devalg_plan(7, 100)
            assert e.value.code == blz.EINVAL and "BLZ_DEVOP_DOT" in str(e.value)
            for nterms in (0, blz.MAX_TERMS + 1):
                with pytest.raises(blz.BlzError) as e:
                    c8.devalg_plan(blz.DEVOP_COMBINE, 100, nterms)
                assert e.value.code == blz.EINVAL and "nterms" in str(e.value)
    with environment(BLZ_DEV_MFMA_MIN_ROWS=None, BLZ_NO_MFMA=None):     # the default thresholds
        for n in (8, 16):
            with blz.Context(P61, n) as ctx:
                for op in ops:
                    plan = ctx.devalg_plan(op, 16, 2)
                    assert plan["form"] == 0 and plan["min_rows"] > 16
    with environment(BLZ_DEV_MFMA_MIN_ROWS="1000", BLZ_NO_MFMA=None):
        with blz.Context(P61, 16) as ctx:
            assert [ctx.devalg_plan(blz.DEVOP_COMBINE, r)["form"] for r in (999, 1000)] == [0, 1]


# ------------------------------------------------------------------------------------------ F. whole iterations


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n", (8, 16))
def test_the_iteration_rebuilt_on_the_matrix_cores(n, right):
    """apply_pair, dot_pair, ortho_coeffs, combine_pair in place, three steps, word for word blz_iterate on a twin context"""
    with environment(BLZ_DEV_MFMA_MIN_ROWS="0", BLZ_NO_MFMA=None):
        with blz.Context(P61, n) as ctx:
            for rows in (200, 300):                     # the two sides of rand300x200
                assert ctx.devalg_plan(blz.DEVOP_DOT_PAIR, rows)["form"] == 1
                assert ctx.devalg_plan(blz.DEVOP_COMBINE_PAIR, rows, 3)["form"] == 1
        F.four_calls_against_twin(n, P61, right, 3, deficient=False)


# ------------------------------------------------------------------------------------------ G. ranks


@pytest.mark.parametrize("n", (8, 16))
def test_rank_local_dot_pair_on_the_matrix_cores(n, monkeypatch):
    """two loopback ranks, 257 rows on one and none on the other: the rank with rows takes the matrix-core form and every
    rank holds the single-rank words"""
    monkeypatch.setenv("BLZ_LOOP_TIMEOUT_S", "20")
    monkeypatch.setenv("BLZ_DEV_MFMA_MIN_ROWS", "0")
    monkeypatch.delenv("BLZ_NO_MFMA", raising=False)
    counts = (257, 0)
    V, AV = R.cycle_block(257, n, 2).reshape(257, n), R.cycle_block(257, n, 9).reshape(257, n)
    vtav, vtaav = (mat(w, n) for w in R.cycle_dot(257, n, 2, 9))

    def body(ctx, g):
        forms = [ctx.devalg_plan(blz.DEVOP_DOT_PAIR, counts[g])["form"], ctx.devalg_plan(blz.DEVOP_DOT, counts[g])["form"]]
        v, av = K.to_dev(V[:counts[g]], 0)[0], K.to_dev(AV[:counts[g]], 2)[0]
        return forms, F.to_host(ctx.dot_pair(v, av, av)), F.to_host(ctx.dot(v, av))

    got = K.on_ranks(2, P61, n, body)
    assert got[0][0] == [1, 1] and got[1][0] == [0, 0]
    for g in range(2):
        assert np.array_equal(got[g][1][0], vtav) and np.array_equal(got[g][1][1], vtaav) and np.array_equal(got[g][2], vtav)
