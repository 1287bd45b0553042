"""Device blocks on several ranks: with blz_set_device_ranks the blocks of the device-block family are a
rank's own rows in slab order, apply and dot are collective, and the default does not move.

Truth is Python integers (exact_ref, rhs_block_ref) and a one-rank twin context; the ranks are loopback ranks, threads of one
process on one GPU as in tests/test_gpu_rhs_ranks.py; every comparison is equality of u64 words.  The matrices are quirks40x30
(an empty row and an empty column; with 8 ranks some ranks own few rows or none) and rand300x200.

1. the numbering          2. take / put              3. apply and apply_pair on ranks     4. dot and dot_pair on ranks
5. the iteration rebuilt  6. the solve left alone    7. the bordered operator             8. one plain rank, mode on
9. what is refused        10. a real communicator on two devices
"""
import ctypes as C
import functools
import os
import threading
import time

import numpy as np
import pytest
import torch

import blz
import exact_ref as X
import rhs_block_ref as RB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P16, P31, P61 = 65537, (1 << 31) - 1, (1 << 61) - 1
P61B, P62 = 2305843009213693907, 4611686018427387847    # Barrett just below 2^61 (8 p <= 2^64 holds) and just below 2^62 (3 p does)
P61C = (1 << 61) - 31
PRIMES = (P16, P31, P61, P61B, P62)
PIDS = {P16: "p16", P31: "p31", P61: "p61", P61B: "p61b", P62: "p62", P61C: "p61c"}
ON_RANKS = [(p, r) for p in PRIMES for r in (2, 3, 8) if r * p <= 1 << 64]
SENTINEL = 0xDEADBEEFCAFEF00D
NAMES = ("quirks40x30", "rand300x200")
NDEV = blz.device_count()


@pytest.fixture(autouse=True)
def short_timeout(monkeypatch):
    """a mismatched collective ends in seconds as BLZ_ECOMM (read when a loopback group is made)"""
    monkeypatch.setenv("BLZ_LOOP_TIMEOUT_S", "20")


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


@functools.lru_cache(maxsize=None)
def pair(name, p):
    return blz.Matrix.load(path(name), p), X.load_mtx(path(name), p)


def run_ranks(nranks, fn):
    """fn(rank) in one thread per rank; the first exception of any rank is re-raised"""
    errs = [None] * nranks

    def go(g):
        try:
            fn(g)
        except BaseException as e:          # noqa: BLE001 (re-raised below)
            errs[g] = e

    ths = [threading.Thread(target=go, args=(g,)) for g in range(nranks)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(600)
    for e in errs:
        if e is not None:
            raise e


def on_ranks(nranks, p, n, body, mode=True, attach=None, devices=False):
    """body(ctx, rank) on nranks contexts, one thread each, joined by a loopback group (or by attach(ctx, rank)); the list of
    what the ranks returned"""
    group = blz.LoopGroup(nranks) if attach is None else None
    out = [None] * nranks

    def rank_main(g):
        with blz.Context(p, n, g if devices else 0) as ctx:
            if attach is None:
                ctx.comm_init_loopback(group, g)
            else:
                attach(ctx, g)
            if mode:
                ctx.device_ranks()
            out[g] = body(ctx, g)
            ctx.sync()

    try:
        run_ranks(nranks, rank_main)
    finally:
        if group is not None:
            group.close()
    return out


def to_dev(w, pad=0, dev="cuda:0"):
    """(view of shape (rows, n) with row stride n + pad, the base tensor) on the device; the padding holds the sentinel"""
    w = np.ascontiguousarray(w, dtype=np.uint64)
    base = np.full((w.shape[0], w.shape[1] + pad), SENTINEL, dtype=np.uint64)
    base[:, :w.shape[1]] = w
    tb = torch.from_numpy(base.view(np.int64)).to(dev)
    return tb[:, :w.shape[1]], tb


def to_host(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def padding_intact(base, n):
    return bool((to_host(base)[:, n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def operand(kind, rows, n, p, seed):
    """a whole block: random residues with 0 and p - 1 planted, or p - 1 throughout; made once, never changed"""
    if kind == "max":
        w = np.full((rows, n), p - 1, dtype=np.uint64)
    else:
        rng = np.random.default_rng([seed, rows, n])
        w = rng.integers(0, p, size=(rows, n), dtype=np.uint64)
        if rows:
            w[rng.integers(0, rows, 2)] = 0
            w[rng.integers(0, rows, 2)] = p - 1
    w.setflags(write=False)
    return w


def ints(a):
    return [int(w) for w in np.asarray(a).reshape(-1)]


def product_ref(Mx, w, transpose, n, p):
    return np.array(X.spmv(Mx, ints(w), transpose, n, p), dtype=np.uint64).reshape(-1, n)


@functools.lru_cache(maxsize=None)
def product_of(name, p, n, transpose, kind):
    """(x, M x or M^T x) on a whole block in the original numbering, in Python integers"""
    Mx = pair(name, p)[1]
    w = operand(kind, Mx.nrows if transpose else Mx.ncols, n, p, 31 + int(transpose))
    return w, product_ref(Mx, w, transpose, n, p)


def x_block(right, transpose):
    """the block whose rows x of y = M x / M^T x has"""
    return blz.V if bool(transpose) != bool(right) else blz.TMP


def whole(parts, rows, n):
    """the ranks' (ids, local rows) put together; every row must come from exactly one rank"""
    full = np.zeros((rows, n), dtype=np.uint64)
    seen = np.zeros(rows, dtype=np.int64)
    for ids, loc in parts:
        assert loc.shape == (len(ids), n), (loc.shape, len(ids))
        full[ids] = loc
        seen[ids] += 1
    assert (seen == 1).all()
    return full


# ------------------------------------------------------------------------------------------ 1. the numbering


@pytest.mark.parametrize("reorder", (True, False), ids=("reordered", "file_order"))
@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("nranks", (1, 2, 3, 8))
def test_the_ids_partition_the_rows(monkeypatch, nranks, right, reorder):
    if not reorder:
        monkeypatch.setenv("BLZ_NO_REORDER", "1")
    if nranks == 1:
        monkeypatch.setenv("BLZ_FORCE_COMM", "1")
    p, n = P61, 8
    for name in NAMES:
        M = pair(name, p)[0]

        def body(ctx, g):
            ctx.set_matrix(M, right, g, nranks)
            rec = {}
            for b in (blz.V, blz.TMP, blz.AV, blz.P):
                first, count = ctx.local_rows(b)
                ids = ctx.local_row_ids(b)
                assert ids.dtype == np.int64 and len(ids) == count
                assert all(ctx.owner_of_row(b, int(r)) == g for r in ids)
                rec[b] = (first, ids, ctx.rows(b))
            assert np.array_equal(rec[blz.V][1], rec[blz.AV][1]) and np.array_equal(rec[blz.V][1], rec[blz.P][1])
            assert ctx.apply_rows(False) == tuple(len(rec[x_block(right, False) ^ q][1]) for q in (0, 1))
            return rec

        got = on_ranks(nranks, p, n, body)
        for b in (blz.V, blz.TMP):
            rows = got[0][b][2]
            assert rows == ((M.ncols if right else M.nrows) if b == blz.V else (M.nrows if right else M.ncols))
            assert sorted(np.concatenate([rec[b][1] for rec in got]).tolist()) == list(range(rows))
            if nranks == 1 and not reorder:             # the file's numbering
                assert np.array_equal(got[0][b][1], np.arange(rows))


# ------------------------------------------------------------------------------------------ 2. take / put


@pytest.mark.parametrize("n", (8, 3, 1))
@pytest.mark.parametrize("nranks", (1, 3))
def test_take_and_put_move_the_ranks_rows_and_nothing_else(nranks, n):
    """strides n, n + 2 and n + 3 on either side: the 16-byte lanes (n = 8, even strides) and the 8-byte ones"""
    p = P61
    M = pair("rand300x200", p)[0]

    def body(ctx, g):
        ctx.set_matrix(M, False, g, nranks)
        for b in (blz.V, blz.TMP):
            rows, ids = ctx.rows(b), ctx.local_row_ids(b)
            W = operand("random", rows, n, p, 5 + b)
            others = np.setdiff1d(np.arange(rows), ids)
            for padw, padl in ((0, 0), (2, 2), (3, 0), (0, 3), (2, 3)):
                w, wbase = to_dev(W, padw)
                loc, lbase = to_dev(np.full((len(ids), n), SENTINEL, dtype=np.uint64), padl)
                assert ctx.take_local(b, w, out=loc) is loc
                assert np.array_equal(to_host(loc), W[ids]) and padding_intact(lbase, n)
                assert np.array_equal(to_host(wbase)[:, :n], W) and padding_intact(wbase, n)
                z, zbase = to_dev(np.full((rows, n), SENTINEL, dtype=np.uint64), padw)
                ctx.put_local(b, loc, z)
                back = to_host(z)
                assert np.array_equal(back[ids], W[ids]) and (back[others] == SENTINEL).all() and padding_intact(zbase, n)
                assert padding_intact(lbase, n)
            # the round trip into the block it came from changes nothing; a fresh local tensor when none is given
            w = to_dev(W)[0].contiguous()
            ctx.put_local(b, ctx.take_local(b, w), w)
            assert np.array_equal(to_host(w), W)
        return True

    assert all(on_ranks(nranks, p, n, body))


@pytest.mark.parametrize("p", (P61, P16), ids=("p61", "p16"))
def test_set_and_get_block_device_move_the_ranks_rows(p):
    """rank-local rows to and from the slab, identity order: blz_get_block (host, original numbering) sees them where the ids
    say; `bad` counts this rank's words only"""
    n, nranks = 3, 3
    M = pair("rand300x200", p)[0]

    def body(ctx, g):
        ctx.set_matrix(M, True, g, nranks)
        for b in (blz.V, blz.TMP, blz.P):
            rows, ids = ctx.rows(b), ctx.local_row_ids(b)
            W = operand("random", rows, n, p, 20 + b)
            loc, lbase = to_dev(W[ids], 2)
            assert ctx.set_block_device(b, loc, validate=True) == 0
            host = ctx.get_block(b).reshape(rows, n)
            assert np.array_equal(host[ids], W[ids]) and padding_intact(lbase, n)
            out, obase = to_dev(np.full((len(ids), n), SENTINEL, dtype=np.uint64), 3)
            ctx.get_block_device(b, out=out)
            assert np.array_equal(to_host(out), W[ids]) and padding_intact(obase, n)
        bad = W[ids].copy()
        bad[g::7, 0] = p + g                            # a different count on every rank
        want = len(bad[g::7])
        with pytest.raises(blz.BlzError) as err:
            ctx.set_block_device(blz.V, to_dev(bad)[0].contiguous(), validate=True)
        assert err.value.code == blz.EINVAL and f"{want} words" in str(err.value), (want, str(err.value))
        return True

    assert all(on_ranks(nranks, p, n, body))


# ------------------------------------------------------------------------------------------ 3. apply on ranks


def apply_cases(ctx, g, nranks, set_matrix, p, n, products):
    """every product of `products` (name, right, M or None -> set, kind, transpose -> truth key) on this rank's rows"""
    rec = {}
    for (name, right), kinds in products.items():
        set_matrix(ctx, name, right, g, nranks)
        ids = {b: ctx.local_row_ids(b) for b in (blz.V, blz.TMP)}
        for kind, (xs, _) in kinds.items():
            for t in (False, True):
                xb = x_block(right, t)
                yb = blz.V + blz.TMP - xb
                assert ctx.apply_rows(t) == (len(ids[xb]), len(ids[yb]))
                x, xbase = to_dev(xs[t][ids[xb]], 2 if t else 3)
                y, ybase = to_dev(np.full((len(ids[yb]), n), SENTINEL, dtype=np.uint64), 3 if t else 0)
                ctx.apply(t, x, out=y)
                assert padding_intact(ybase, n) and np.array_equal(to_host(xbase)[:, :n], xs[t][ids[xb]])
                rec[(name, right, kind, "apply", t)] = (ids[yb], to_host(y))
            # z = op2 (op1 x) from the side of v: with the intermediate, without it, in place
            t = not right
            x = to_dev(xs[t][ids[blz.V]])[0].contiguous()
            z, mid = ctx.apply_pair(t, x, mid=True)
            rec[(name, right, kind, "pair_mid", t)] = (ids[blz.TMP], to_host(mid))
            rec[(name, right, kind, "pair", t)] = (ids[blz.V], to_host(z))
            z2 = ctx.apply_pair(t, x)
            assert ctx.apply_pair(t, x, out=x) is x
            assert np.array_equal(to_host(z2), to_host(z)) and np.array_equal(to_host(x), to_host(z))
    return rec


def check_apply(got, products, n, p):
    for (name, right), kinds in products.items():
        for kind, (xs, want) in kinds.items():
            for t in (False, True):
                have = whole([rec[(name, right, kind, "apply", t)] for rec in got], want[t].shape[0], n)
                assert np.array_equal(have, want[t]), (name, right, kind, t, np.argwhere(have != want[t])[:3])
            t = not right
            mid = whole([rec[(name, right, kind, "pair_mid", t)] for rec in got], want[t].shape[0], n)
            assert np.array_equal(mid, want[t]), (name, right, kind, "mid")
            z = whole([rec[(name, right, kind, "pair", t)] for rec in got], want["pair"].shape[0], n)
            assert np.array_equal(z, want["pair"]), (name, right, kind, "pair")


@functools.lru_cache(maxsize=None)
def plain_products(p, n):
    """{(name, right): {kind: ({t: x}, {t: M x / M^T x, "pair": op2 (op1 x)})}} for both matrices, in Python integers"""
    out = {}
    for name in NAMES:
        Mx = pair(name, p)[1]
        for right in (False, True):
            kinds = {}
            for kind in ("random", "max"):
                xs = {t: product_of(name, p, n, t, kind)[0] for t in (False, True)}
                want = {t: product_of(name, p, n, t, kind)[1] for t in (False, True)}
                t = not right
                want["pair"] = product_ref(Mx, want[t], not t, n, p)
                kinds[kind] = (xs, want)
            out[(name, right)] = kinds
    return out


@pytest.mark.parametrize("n", (1, 3, 8, 16))
@pytest.mark.parametrize("p, nranks", ON_RANKS, ids=[f"{PIDS[p]}-r{r}" for p, r in ON_RANKS])
def test_apply_on_ranks_against_exact_integers(monkeypatch, p, nranks, n):
    """both products, both kernels' sides, random operands and p - 1 throughout, the exchange in one piece and in two;
    apply_pair with the intermediate, without it and in place"""
    products = plain_products(p, n)

    def set_matrix(ctx, name, right, g, nr):
        ctx.set_matrix(pair(name, p)[0], right, g, nr)

    for chunks in (1, 2):
        monkeypatch.setenv("BLZ_AG_CHUNKS", str(chunks))

        def body(ctx, g):
            rec = apply_cases(ctx, g, nranks, set_matrix, p, n, products)
            assert ctx.exchange_pieces(False) == chunks and ctx.exchange_pieces(True) == chunks
            return rec

        check_apply(on_ranks(nranks, p, n, body), products, n, p)


# ------------------------------------------------------------------------------------------ 4. dot on ranks

ROWS = (257, 0, 1000, 1)        # rank g holds ROWS[g % 4] rows: unequal, and some ranks hold none


def gram(A, B, p, n):
    if A.shape[0] == 0:
        return np.zeros((n, n), dtype=np.uint64)
    return np.array((A.astype(object).T @ B.astype(object)) % p, dtype=np.uint64).reshape(n, n)


@pytest.mark.parametrize("n", (1, 3, 8, 16))
@pytest.mark.parametrize("p, nranks", ON_RANKS, ids=[f"{PIDS[p]}-r{r}" for p, r in ON_RANKS])
def test_dot_on_ranks_is_the_sum_over_all_rows(p, nranks, n):
    """no matrix: the ranks are the communicator's.  At 8 ranks and p - 1 throughout the all-reduce carries the largest sums"""
    counts = [ROWS[g % 4] for g in range(nranks)]
    blocks = {kind: [[operand(kind, counts[g], n, p, 100 + 10 * g + q) for q in range(3)] for g in range(nranks)]
              for kind in ("random", "max")}

    def body(ctx, g):
        rec = {}
        for kind in ("random", "max"):
            a, b, c = (to_dev(w, pad)[0] for w, pad in zip(blocks[kind][g], (0, 2, 3)))
            out = torch.full((n, n), -1, dtype=torch.int64, device="cuda:0")
            assert ctx.dot(a, b, out=out) is out
            rec[kind] = [to_host(out), to_host(ctx.dot(a, a)), to_host(ctx.dot_pair(a, b, c)), to_host(ctx.dot_pair(b, c, c))]
        return rec

    got = on_ranks(nranks, p, n, body)
    for kind in ("random", "max"):
        A, B, Cc = (np.concatenate([blocks[kind][g][q] for g in range(nranks)]) for q in range(3))
        want = [gram(A, B, p, n), gram(A, A, p, n), np.stack([gram(A, Cc, p, n), gram(B, Cc, p, n)]),
                np.stack([gram(B, Cc, p, n), gram(Cc, Cc, p, n)])]
        for g in range(nranks):                         # every rank holds the same words
            for have, w in zip(got[g][kind], want):
                assert np.array_equal(have, w), (kind, g)


# ------------------------------------------------------------------------------------------ 5. the iteration rebuilt on ranks


def fused_step(ctx, right, v, pb):
    """sequential/lanczos_modp.c:635-656 in four calls on the rank's rows, v and p updated in place"""
    Av = ctx.apply_pair(not right, v)
    c = ctx.dot_pair(v, Av, Av)                         # vtAv, vtAAv: summed over the ranks
    coef, npiv = ctx.ortho_coeffs(c[0], c[1])
    ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))
    return c


@pytest.mark.parametrize("nranks", (1, 2, 3))
@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ((8, P61), (3, P16), (16, P61C)), ids=("n8p61", "n3p16", "n16p61c"))
def test_the_iteration_rebuilt_on_ranks(monkeypatch, n, p, right, nranks):
    steps = 6
    M = pair("rand300x200", p)[0]
    with blz.Context(p, n) as twin:                     # one plain rank, blz_iterate
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v0 = twin.get_block(blz.V).reshape(rows, n)
        want = []
        for _ in range(steps):
            assert twin.iterate(1)[:2] == (1, False)
            want.append((twin.get_small(blz.VTAV), twin.get_small(blz.VTAAV), twin.get_block(blz.V), twin.get_block(blz.P)))
    if nranks == 1:
        monkeypatch.setenv("BLZ_FORCE_COMM", "1")

    def body(ctx, g):
        ctx.set_matrix(M, right, g, nranks)
        ids = ctx.local_row_ids(blz.V)
        v = torch.empty((len(ids), n), dtype=torch.int64, device="cuda:0")
        ctx.take_local(blz.V, to_dev(v0)[0].contiguous(), out=v)
        pb = torch.zeros_like(v)
        got = []
        for _ in range(steps):                          # no tensor is read on the host in here
            c = fused_step(ctx, right, v, pb)           # (c: a new tensor every step)
            got.append((c, v.clone(), pb.clone()))
        assert ctx.iterations == 0
        return ids, [tuple(to_host(t) for t in rec) for rec in got]

    got = on_ranks(nranks, p, n, body)
    for step, (wA, wAA, wv, wp) in enumerate(want):
        for ids, rec in got:
            assert np.array_equal(rec[step][0][0].reshape(-1), wA) and np.array_equal(rec[step][0][1].reshape(-1), wAA), step
        assert np.array_equal(whole([(ids, rec[step][1]) for ids, rec in got], rows, n).reshape(-1), wv), step
        assert np.array_equal(whole([(ids, rec[step][2]) for ids, rec in got], rows, n).reshape(-1), wp), step


# ------------------------------------------------------------------------------------------ 6. the solve left alone


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def foreign_calls(ctx, g, n, p, right):
    """every device call of the family on tensors that have nothing to do with the solve (each rank makes the same calls in
    the same order: five of them are collective)"""
    vr, tr = ctx.local_rows(blz.V)[1], ctx.local_rows(blz.TMP)[1]
    a, b = (to_dev(operand("random", vr, n, p, 70 + 5 * g + q))[0].contiguous() for q in range(2))
    t = to_dev(operand("random", tr, n, p, 80 + g))[0].contiguous()
    y = ctx.apply(not right, a)                         # from the side of v, then from the other side
    ctx.apply(right, t)
    z, mid = ctx.apply_pair(not right, a, mid=True)
    assert np.array_equal(to_host(mid), to_host(y))
    c = ctx.dot_pair(a, z, z)
    d = ctx.dot(a, b)
    coef, _ = ctx.ortho_coeffs(c[0], c[1])
    ctx.semi_inverse_device(d)
    ctx.combine([(a, coef[0]), (b, coef[1])], out=b)
    ctx.combine_pair([(z, coef[blz.COEF_V_AV], None), (a, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (b, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(a, b))
    W = to_dev(operand("random", ctx.rows(blz.V), n, p, 90))[0].contiguous()
    ctx.put_local(blz.V, ctx.take_local(blz.V, W), W)
    return to_host(c)


def test_the_calls_on_ranks_leave_the_solve_alone():
    p, n, nranks, right = P61, 8, 2, False
    M = pair("rand300x200", p)[0]

    def solve(disturb):
        def body(ctx, g):
            ctx.set_matrix(M, right, g, nranks)
            ctx.init_v()
            trail = []
            if disturb:
                trail.append(foreign_calls(ctx, g, n, p, right))
            stopped = False
            while not stopped:
                stopped = ctx.iterate(5)[1]
                if disturb:
                    trail.append(foreign_calls(ctx, g, n, p, right))
            return state(ctx) + [np.array(ctx.final_check())], trail
        return on_ranks(nranks, p, n, body, mode=disturb)

    twin, got = solve(False), solve(True)
    assert int(twin[0][0][8][0]) > 5                    # several batches
    for g in range(nranks):
        assert len(got[g][0]) == len(twin[g][0]) and all(np.array_equal(s, t) for s, t in zip(got[g][0], twin[g][0])), g
        assert len(got[g][1]) >= 3 and all(np.array_equal(c, got[0][1][0]) for c in got[g][1])    # the same sums, every time, every rank


# ------------------------------------------------------------------------------------------ 7. the bordered operator


@functools.lru_cache(maxsize=None)
def bordered_products(p, n, k):
    out = {}
    Mx = pair("quirks40x30", p)[1]
    for right in (False, True):
        cols = [ints(operand("random", Mx.nrows if right else Mx.ncols, 1, p, 40 + i)) for i in range(k)]
        A = RB.augmented(Mx, cols, right)
        kinds = {}
        for kind in ("random", "max"):
            xs = {t: operand(kind, A.nrows if t else A.ncols, n, p, 45 + int(t)) for t in (False, True)}
            want = {t: product_ref(A, xs[t], t, n, p) for t in (False, True)}
            want["pair"] = product_ref(A, want[not right], right, n, p)
            kinds[kind] = (xs, want)
        out[("quirks40x30", right)] = kinds
        out[("cols", right)] = RB.rows(cols)
    return out


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("nranks", (2, 3))
def test_apply_on_ranks_is_the_bordered_operator(nranks, k):
    p, n = P61, 4
    Mb = pair("quirks40x30", p)[0]
    prods = bordered_products(p, n, k)
    products = {key: val for key, val in prods.items() if key[0] != "cols"}

    def set_matrix(ctx, name, right, g, nr):
        ctx.set_matrix_rhs_ranks(Mb, prods[("cols", right)], right, g, nr)
        assert ctx.has_rhs and ctx.rhs_count == k

    check_apply(on_ranks(nranks, p, n, lambda ctx, g: apply_cases(ctx, g, nranks, set_matrix, p, n, products)), products, n, p)


# ------------------------------------------------------------------------------------------ 8. one plain rank, mode on


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
def test_one_plain_rank_with_the_mode_on(right):
    """take, apply, put = apply in the original numbering with the mode off; the switch goes both ways on one context"""
    p, n = P61, 8
    M = pair("rand300x200", p)[0]
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M, right)
        assert not ctx.device_ranks_on
        for t in (False, True):
            xb = x_block(right, t)
            yb = blz.V + blz.TMP - xb
            x = to_dev(operand("random", ctx.rows(xb), n, p, 60 + int(t)))[0].contiguous()
            want = ctx.apply(t, x)
            assert ctx.device_ranks() is ctx and ctx.device_ranks_on
            assert ctx.local_rows(xb) == (0, ctx.rows(xb)) and ctx.apply_rows(t) == (ctx.rows(xb), ctx.rows(yb))
            y = torch.full((ctx.rows(yb), n), -1, dtype=torch.int64, device="cuda:0")
            ctx.put_local(yb, ctx.apply(t, ctx.take_local(xb, x)), y)
            assert torch.equal(y.view(torch.uint64), want.view(torch.uint64))
            e, _, info = ctx.rref(x)                    # the echelon stays allowed on a plain single rank
            assert int(info[0]) == n
            # the dot is today's path: no communicator, no collective
            assert torch.equal(ctx.dot(x, x).view(torch.int64), ctx.device_ranks(False).dot(x, x).view(torch.int64))
            assert not ctx.device_ranks_on


# ------------------------------------------------------------------------------------------ 9. what is refused


def refusal(call):
    with pytest.raises(blz.BlzError) as err:
        call()
    return err.value.code, str(err.value)


def test_mode_off_keeps_todays_refusal_on_ranks():
    p, n = P61, 8
    M = pair("rand300x200", p)[0]
    x = to_dev(operand("random", M.nrows, n, p, 1))[0].contiguous()

    def body(ctx, g):
        ctx.set_matrix(M, False, g, 2)
        assert not ctx.device_ranks_on
        for call in (lambda: ctx.dot(x, x), lambda: ctx.dot_pair(x, x, x), lambda: ctx.combine([(x, np.eye(n, dtype=np.uint64))]),
                     lambda: ctx.rref(x)):
            code, msg = refusal(call)
            assert code == blz.EINVAL and "single rank" in msg, msg
        code, msg = refusal(lambda: ctx.take_local(blz.V, x))
        assert code == blz.EINVAL and "blz_set_device_ranks" in msg, msg
        return True

    assert all(on_ranks(2, p, n, body, mode=False))


def test_refusals_on_ranks_are_named_and_nobody_waits(monkeypatch):
    """every rank refuses before the first enqueue and before any rendezvous: the outputs keep the sentinel and the test is
    over long before a time-out of the group could have run out"""
    n = 8
    t0 = time.monotonic()

    def sentinel(*shape):
        return torch.from_numpy(np.full(shape, SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool((to_host(t) == SENTINEL).all()) for t in ts)

    # the echelon on ranks; a block of the wrong local row count
    M = pair("rand300x200", P61)[0]

    def body(ctx, g):
        ctx.set_matrix(M, False, g, 2)
        x = to_dev(operand("random", ctx.local_rows(blz.V)[1], n, P61, 1))[0].contiguous()
        code, msg = refusal(lambda: ctx.rref(x))
        assert code == blz.EINVAL and "echelon on ranks is not built" in msg, msg
        full, y = to_dev(operand("random", ctx.rows(blz.V), n, P61, 2))[0].contiguous(), sentinel(ctx.local_rows(blz.TMP)[1], n)
        with pytest.raises(ValueError) as e:
            ctx.apply(True, full, out=y)
        assert f"{ctx.rows(blz.V)} rows, the block has {ctx.local_rows(blz.V)[1]}" in str(e.value)
        with pytest.raises(ValueError):
            ctx.set_block_device(blz.V, full)
        code, msg = refusal(lambda: ctx.set_exchange_mode(True))
        assert code == blz.EINVAL and "blz_set_device_ranks" in msg, msg
        return untouched(y)

    assert all(on_ranks(2, P61, n, body))

    # external exchange, set before the mode
    def body(ctx, g):
        x, c = to_dev(operand("random", 40, n, P61, 1))[0].contiguous(), sentinel(n, n)
        code, msg = refusal(lambda: ctx.dot(x, x, out=c))
        assert code == blz.EINVAL and "external-exchange" in msg, msg
        return untouched(c)

    def external(ctx, g):
        ctx.set_exchange_mode(True)
        ctx.device_ranks()
        return body(ctx, g)

    assert all(on_ranks(2, P61, n, external, mode=False))

    # the short-side form of a tall matrix
    monkeypatch.setenv("BLZ_SHORT_SIDE", "1")
    tall = blz.Matrix.synth(600, 40, 2400, 0x54414C4C, P61)

    def body(ctx, g):
        ctx.set_matrix(tall, False, g, 2)
        assert ctx.short_side(False) or ctx.short_side(True)
        xr, yr = ctx.apply_rows(False)
        x, y, z = to_dev(operand("random", xr, n, P61, 3))[0].contiguous(), sentinel(yr, n), sentinel(xr, n)
        for call in (lambda: ctx.apply(False, x, out=y), lambda: ctx.apply_pair(False, x, out=z)):
            code, msg = refusal(call)
            assert code == blz.EINVAL and "short-side" in msg, msg
        return untouched(y, z)

    assert all(on_ranks(2, P61, n, body))
    monkeypatch.delenv("BLZ_SHORT_SIDE")

    # 8 ranks at a prime just below 2^62: the sum of 8 residues may wrap
    def body(ctx, g):
        x, c, c2 = to_dev(operand("random", 40, n, P62, 1))[0].contiguous(), sentinel(n, n), sentinel(2, n, n)
        for call in (lambda: ctx.dot(x, x, out=c), lambda: ctx.dot_pair(x, x, x, out=c2)):
            code, msg = refusal(call)
            assert code == blz.EINVAL and "nranks * p" in msg, msg
        return untouched(c, c2)

    assert all(on_ranks(8, P62, n, body))
    assert time.monotonic() - t0 < 15, "somebody waited at a rendezvous"


def test_a_capturing_stream_is_refused_with_the_mode_on():
    p, n = P61, 8
    M = pair("rand300x200", p)[0]
    group = blz.LoopGroup(1)
    try:
        with blz.Context(p, n) as ctx:
            ctx.comm_init_loopback(group, 0)
            ctx.device_ranks()
            ctx.set_matrix(M)
            rows = ctx.rows(blz.V)
            x = to_dev(operand("random", rows, n, p, 1))[0].contiguous()
            w = torch.from_numpy(np.full((rows, n), SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")
            c = torch.from_numpy(np.full((n, n), SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")
            ctx.take_local(blz.V, x)                    # (the numbering is on the device before anything is captured)
            L, h = blz.lib(), ctx.h
            s = torch.cuda.Stream(device="cuda:0")
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):         # captured and thrown away: never replayed
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                X_, W_, C_ = (C.c_void_p(t.data_ptr()) for t in (x, w, c))
                ld, rws = C.c_int64(n), C.c_int64(rows)
                rcs, msgs = [], []
                for call in (lambda: L.blz_dot_device(h, rws, X_, ld, X_, ld, C_, st),
                             lambda: L.blz_apply_pair_device(h, C.c_int(0), X_, ld, None, ld, W_, ld, st),
                             lambda: L.blz_take_local_device(h, C.c_int(blz.V), X_, ld, W_, ld, st),
                             lambda: L.blz_put_local_device(h, C.c_int(blz.V), X_, ld, W_, ld, st)):
                    rcs.append(call())
                    msgs.append(L.blz_last_error().decode())
                x.add_(0)                               # (a graph of one node, not an empty one)
            assert rcs == [blz.EINVAL] * 4 and all("capturing" in m for m in msgs), (rcs, msgs)
            torch.cuda.synchronize()
            assert (to_host(w) == SENTINEL).all() and (to_host(c) == SENTINEL).all()
    finally:
        group.close()


# ------------------------------------------------------------------------------------------ 10. a real communicator


@pytest.mark.skipif(NDEV < 2, reason="needs two GPUs")
def test_two_devices_through_the_real_communicator():
    """the same calls over RCCL, one context per device: apply against exact integers, dot against the sum over both ranks"""
    p, n, nranks = P61, 8, 2
    uid = blz.comm_unique_id()
    products = {key: val for key, val in plain_products(p, n).items() if key[0] == "rand300x200"}
    blocks = [[operand("random", ROWS[g], n, p, 200 + 10 * g + q) for q in range(2)] for g in range(nranks)]

    def body(ctx, g):
        dev = f"cuda:{g}"
        with torch.cuda.device(dev):
            rec = {}
            for (name, right), kinds in products.items():
                ctx.set_matrix(pair(name, p)[0], right, g, nranks)
                xs, _ = kinds["random"]
                t = not right
                ids = ctx.local_row_ids(blz.V)
                z = ctx.apply_pair(t, to_dev(xs[t][ids], dev=dev)[0].contiguous())
                rec[right] = (ids, to_host(z))
            a, b = (to_dev(w, dev=dev)[0].contiguous() for w in blocks[g])
            rec["dot"] = to_host(ctx.dot(a, b))
            return rec

    got = on_ranks(nranks, p, n, body, attach=lambda ctx, g: ctx.comm_init(uid, g, nranks), devices=True)
    for (name, right), kinds in products.items():
        want = kinds["random"][1]["pair"]
        assert np.array_equal(whole([rec[right] for rec in got], want.shape[0], n), want), right
    A, B = (np.concatenate([blocks[g][q] for g in range(nranks)]) for q in range(2))
    assert all(np.array_equal(rec["dot"], gram(A, B, p, n)) for rec in got)
