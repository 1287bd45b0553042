"""Device blocks on the GPU: blocks handed over and taken back as torch tensors (blz_set_block_device / blz_get_block_device)
and M or M^T applied to caller-owned device memory (blz_apply_device), against

  - the host path (blz_set_block / blz_get_block), word for word, both ways;
  - the CPU oracle's product (oracle.spmv) for plain contexts;
  - blz_set_block / blz_spmv / blz_get_block on a SECOND context for the signed, the wide and the bordered operator;
  - an undisturbed twin context for "apply leaves the solve alone".

Every comparison is equality of u64 words.  The matrices are the golden ones; each test first asserts through
blz.reorder_auto that its matrix IS renumbered (a permutation that is the identity would let a kernel that ignores it pass).
Tensors are int64 views of the u64 words where torch has to compute on them (same bits), torch.uint64 where the library
allocates.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import blz
import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P61 = (1 << 61) - 1
P61B = (1 << 61) - 31
P16 = 65537
SENTINEL = 0xDEADBEEFCAFEF00D
_M, _O = {}, {}


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


def matrix(name, p):
    """blz.Matrix of a golden file, loaded once and never changed; asserts that the solver renumbers it"""
    if (name, p) not in _M:
        M = blz.Matrix.load(path(name), p)
        rp, cp = blz.reorder_auto(M)[:2]
        assert (rp != np.arange(M.nrows)).any() and (cp != np.arange(M.ncols)).any(), "the renumbering is the identity"
        _M[(name, p)] = M
    return _M[(name, p)]


def oracle_matrix(name, p):
    if (name, p) not in _O:
        _O[(name, p)] = orc.Matrix.load(path(name), p)
    return _O[(name, p)]


def residues(rows, n, p, seed):
    """random residues with 0 and p - 1 in every column"""
    rng = np.random.default_rng([seed, rows, n])
    w = rng.integers(0, p, size=(rows, n), dtype=np.uint64)
    w[rng.integers(0, rows, 3)] = 0
    w[rng.integers(0, rows, 3)] = p - 1
    return w


def to_dev(words, pad=0, fill=SENTINEL):
    """(view of shape (rows, n) with row stride n + pad, the base tensor) on the device, int64 bits of the u64 words"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    base = np.full((words.shape[0], words.shape[1] + pad), fill, dtype=np.uint64)
    base[:, :words.shape[1]] = words
    tb = torch.from_numpy(base.view(np.int64)).to("cuda:0")
    return tb[:, :words.shape[1]], tb


def to_host(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def flat(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


# ------------------------------------------------------------------------------------------ 1. import / export


def roundtrip(ctx, p, n, seed):
    for block in (blz.V, blz.TMP):
        rows = ctx.rows(block)
        for pad in (0, 3):
            words = residues(rows, n, p, seed + 10 * block + pad)
            ctx.set_block(block, np.zeros(rows * n, dtype=np.uint64))
            view, _ = to_dev(words, pad)
            assert view.stride() == (n + pad, 1) or rows == 1 or n == 1
            assert ctx.set_block_device(block, view) is None
            assert np.array_equal(ctx.get_block(block), flat(words)), (block, pad, "device set, host get")
            other = residues(rows, n, p, seed + 100 + 10 * block + pad)
            ctx.set_block(block, flat(other))
            out, base = to_dev(np.zeros((rows, n), dtype=np.uint64), pad)
            got = ctx.get_block_device(block, out=out)
            assert got is out
            host = to_host(base)
            assert np.array_equal(host[:, :n], other), (block, pad, "host set, device get")
            assert (host[:, n:] == SENTINEL).all(), "words past n of a caller's row were written"
        fl = torch.from_numpy(flat(words).view(np.int64)).to("cuda:0")       # the flat layout, and a library-made uint64 tensor
        ctx.set_block_device(block, fl)
        new = ctx.get_block_device(block)
        assert new.dtype == torch.uint64 and tuple(new.shape) == (rows, n)
        assert np.array_equal(to_host(new), words)


@pytest.mark.parametrize("n", (1, 3, 5, 8, 16, 64))
@pytest.mark.parametrize("p", (P16, P61, P61B), ids=("p16", "p61", "p61b"))
def test_import_and_export_against_the_host_path(p, n, monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")        # the matrix-core block update at these sizes: p implicit at n = 8, p = 2^61 - 1
    M = matrix("rand3000x2000", p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M)
        assert ctx.word_bytes == (4 if p < 1 << 32 else 8)
        roundtrip(ctx, p, n, seed=n)
        # P after three iterations, against the host path of a twin that never saw a device call
        twin.set_matrix(M)
        for c in (ctx, twin):
            c.init_v()
            assert c.iterate(3)[0] == 3
        if (p, n) == (P61, 8):
            assert ctx.p_implicit == 1
        got = to_host(ctx.get_block_device(blz.P))
        assert ctx.p_implicit == 0
        assert np.array_equal(got.reshape(-1), twin.get_block(blz.P))
        assert np.array_equal(ctx.get_block(blz.P), twin.get_block(blz.P))
        for b in (blz.V, blz.AV):
            assert np.array_equal(to_host(ctx.get_block_device(b)).reshape(-1), twin.get_block(b))
        # a device set of P makes it explicit, as blz_set_block does
        for c in (ctx, twin):
            c.iterate(2)
        if (p, n) == (P61, 8):
            assert ctx.p_implicit == 1
        words = residues(ctx.rows(blz.P), n, p, seed=77)
        ctx.set_block_device(blz.P, to_dev(words)[0])
        assert ctx.p_implicit == 0
        assert np.array_equal(ctx.get_block(blz.P), flat(words))
        twin.set_block(blz.P, flat(words))
        for c in (ctx, twin):
            c.iterate(2)
        for b in (blz.V, blz.P):
            assert np.array_equal(ctx.get_block(b), twin.get_block(b)), b


def test_exact_width_slabs(monkeypatch):
    monkeypatch.setenv("BLZ_NO_PAD", "1")               # n = 3 words per slab row: not a power of two
    for p in (P16, P61):
        with blz.Context(p, 3) as ctx:
            ctx.set_matrix(matrix("rand3000x2000", p))
            assert ctx.plan(False)["width"] == 3
            roundtrip(ctx, p, 3, seed=5)
            x = residues(2000, 3, p, seed=6)
            y = ctx.apply(False, to_dev(x, 3)[0])
            assert np.array_equal(to_host(y).reshape(-1), orc.spmv(oracle_matrix("rand3000x2000", p), flat(x), False, 3, p))


def test_identity_numbering(monkeypatch):
    monkeypatch.setenv("BLZ_NO_REORDER", "1")           # the permutation arrays are empty
    for name, n in (("quirks40x30", 8), ("rand3000x2000", 5)):
        with blz.Context(P61, n) as ctx:
            M = matrix(name, P61)
            ctx.set_matrix(M)
            roundtrip(ctx, P61, n, seed=9)
            x = residues(M.nrows, n, P61, seed=10)
            y = ctx.apply(True, to_dev(x)[0])
            assert np.array_equal(to_host(y).reshape(-1), orc.spmv(oracle_matrix(name, P61), flat(x), True, n, P61))


def test_the_small_matrices_too():
    """40 and 30 rows with an empty row and column; 120 x 260: fewer rows than one workgroup takes at small n"""
    for name in ("quirks40x30", "wide120x260"):
        for p, n in ((P61, 8), (P16, 2), (P61B, 64)):
            with blz.Context(p, n) as ctx:
                ctx.set_matrix(matrix(name, p))
                roundtrip(ctx, p, n, seed=21)


# ------------------------------------------------------------------------------------------ 2. apply against the oracle


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("p, n", ((P61, 8), (P16, 5), (P61B, 16)), ids=("p61n8", "p16n5", "p61bn16"))
def test_apply_against_the_oracle(p, n, right):
    name = "rand3000x2000"
    M, O = matrix(name, p), oracle_matrix(name, p)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M, right)
        for transpose in (False, True):
            xr, yr = ctx.apply_rows(transpose)
            assert (xr, yr) == ((M.nrows, M.ncols) if transpose else (M.ncols, M.nrows))
            for kind in ("random", "max", "zero"):
                x = (residues(xr, n, p, seed=3) if kind == "random" else
                     np.full((xr, n), p - 1 if kind == "max" else 0, dtype=np.uint64))
                want = orc.spmv(O, flat(x), transpose, n, p)
                y = ctx.apply(transpose, to_dev(x)[0])
                assert tuple(y.shape) == (yr, n) and y.dtype == torch.uint64
                assert np.array_equal(to_host(y).reshape(-1), want), (transpose, kind)
                if kind == "random":
                    assert want.any()
                    out, base = to_dev(np.zeros((yr, n), dtype=np.uint64), 3)       # strided x and y, the caller's out
                    assert ctx.apply(transpose, to_dev(x, 3)[0], out=out) is out
                    host = to_host(base)
                    assert np.array_equal(host[:, :n].reshape(-1), want) and (host[:, n:] == SENTINEL).all()
        ctx.apply_release()
        ctx.apply_release()                             # nothing to free: fine
        y = ctx.apply(False, to_dev(residues(M.ncols, n, p, seed=4))[0])            # and the slabs come back
        assert np.array_equal(to_host(y).reshape(-1), orc.spmv(O, flat(residues(M.ncols, n, p, seed=4)), False, n, p))


# ------------------------------------------------------------------------------------------ 3. apply against spmv on a second context


def spmv_on(ctx, transpose, x):
    """set_block / spmv / get_block: product `not right` reads V and writes TMP, the other reads TMP and writes AV"""
    src, dst = (blz.V, blz.TMP) if bool(transpose) == (not ctx.right) else (blz.TMP, blz.AV)
    ctx.set_block(src, flat(x))
    ctx.spmv(transpose, src, dst)
    return ctx.get_block(dst)


def both_products(make, p, n):
    """apply on one context against spmv_on on another made the same way, both transposes, extremes included"""
    with make() as ctx, make() as ref:
        for transpose in (False, True):
            xr, yr = ctx.apply_rows(transpose)
            assert yr * n == spmv_on(ref, transpose, np.zeros((xr, n), dtype=np.uint64)).size
            for kind in ("random", "max"):
                x = residues(xr, n, p, seed=8) if kind == "random" else np.full((xr, n), p - 1, dtype=np.uint64)
                want = spmv_on(ref, transpose, x)
                assert want.any() or kind == "max"      # (an incidence matrix maps a constant block to zero)
                assert np.array_equal(to_host(ctx.apply(transpose, to_dev(x, 3)[0])).reshape(-1), want), (transpose, kind)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
def test_apply_in_signed_mode(right):
    p, n = P61, 8
    M = blz.Matrix.load_signed(path("graph200x600"))
    assert (M.x.view(np.int32) < 0).any()               # an incidence matrix: -1 among its entries
    assert (blz.reorder_auto(M)[0] != np.arange(M.nrows)).any()

    def make():
        ctx = blz.Context(p, n)
        ctx.set_values_signed()
        ctx.set_matrix(M, right)
        assert ctx.slab_signed(False) and ctx.slab_signed(True)
        return ctx
    both_products(make, p, n)


@pytest.mark.parametrize("p", (P61, P61B), ids=("p61", "p61b"))
def test_apply_in_wide_mode(p):
    n = 4
    base = matrix("rand3000x2000", p)
    hi = np.random.default_rng(12).integers(0, 1 << 28, base.nnz, dtype=np.uint32)     # entries up to 2^60: residues below p
    M = blz.Matrix(base.nrows, base.ncols, base.i, base.j, base.x, x_hi=hi)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix(M, True)
        assert ctx.values_wide() and ctx.slab_wide(False) and ctx.slab_wide(True)
        return ctx
    both_products(make, p, n)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("k", (1, 3))
def test_apply_on_a_bordered_context(k, right):
    p, n = P61, 4
    M = matrix("rand3000x2000", p)
    b = residues(M.nrows if right else M.ncols, k, p, seed=k)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix_rhs_block(M, b, right)
        assert ctx.rhs_count == k
        return ctx
    with make() as ctx:                                 # the border rows count
        assert ctx.apply_rows(not right) == (ctx.rows(blz.V), ctx.rows(blz.TMP))
        assert ctx.rows(blz.V) == (M.ncols if right else M.nrows) + k
    both_products(make, p, n)


# ------------------------------------------------------------------------------------------ 4. the solve is not disturbed


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(s, t) for s, t in zip(a, b))


def test_apply_leaves_the_solve_alone(monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")        # p implicit while the iteration runs
    p, n, name = P61, 8, "rand3000x2000"
    M, O = matrix(name, p), oracle_matrix(name, p)
    xs = {t: residues(M.nrows if t else M.ncols, n, p, seed=31 + t) for t in (False, True)}
    want = {t: orc.spmv(O, flat(xs[t]), t, n, p) for t in (False, True)}
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        for c in (ctx, twin):
            c.set_matrix(M)
            c.init_v()
            assert c.iterate(3)[:2] == (3, False)
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        for t in (False, True):                         # while p is implicit: the flag and the count do not move
            assert np.array_equal(to_host(ctx.apply(t, to_dev(xs[t])[0])).reshape(-1), want[t])
        ctx.apply_release()
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        before = state(ctx)                             # (looking at P makes it explicit)
        assert same(before, state(twin))
        for t in (False, True):                         # and the literal form: record, apply twice, release, compare
            assert np.array_equal(to_host(ctx.apply(t, to_dev(xs[t])[0])).reshape(-1), want[t])
        ctx.apply_release()
        assert ctx.p_implicit == 0 and same(before, state(ctx))
        stopped = False
        while not stopped:                              # on to the stop, an apply between the batches
            stopped = ctx.iterate(64)[1]
            assert twin.iterate(64)[1] == stopped
            ctx.apply(False, to_dev(xs[False])[0])
        assert ctx.iterations == twin.iterations > 3
        assert same(state(ctx), state(twin))
        assert ctx.final_check() == twin.final_check()
        for t in (False, True):                         # past the stop every kernel of the solve is a no-op; apply is not
            out, _ = to_dev(np.full((ctx.apply_rows(t)[1], n), SENTINEL, dtype=np.uint64))
            ctx.apply(t, to_dev(xs[t])[0], out=out)
            assert want[t].any() and np.array_equal(to_host(out).reshape(-1), want[t])
        assert same(state(ctx), state(twin))


# ------------------------------------------------------------------------------------------ 5. stream order


def test_apply_is_ordered_on_the_callers_stream():
    p, n, name = P61, 8, "rand3000x2000"
    M, O = matrix(name, p), oracle_matrix(name, p)
    a, b = residues(M.ncols, n, p, seed=41), residues(M.ncols, n, p, seed=42)
    x_host = (a.astype(object) + b.astype(object)) % p
    want = (orc.spmv(O, flat(np.array(x_host, dtype=np.uint64)), False, n, p).astype(object) + 1) % p
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        ctx.apply(False, to_dev(a)[0])                  # (scratch slabs and numbering are in place: nothing synchronous is left)
        ta, tb = to_dev(a)[0].contiguous(), to_dev(b)[0].contiguous()
        big = torch.rand(2048, 2048, device="cuda:0")
        out = torch.full((M.nrows, n), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            for _ in range(20):                         # a few milliseconds of work ahead of x on this stream
                big = torch.nn.functional.normalize(big @ big)
            x = torch.remainder(ta + tb + (big[0, 0] > 2).to(torch.int64), p)      # (a + b) mod p, behind the products above
            y = ctx.apply(False, x, out=out)            # stream=None: torch's current stream, which is s
            z = torch.remainder(y + 1, p)               # consumed at once
            got = z.cpu().numpy().view(np.uint64)       # the only synchronisation: this copy, on s
    assert np.array_equal(got.reshape(-1), np.array(want, dtype=np.uint64))


# ------------------------------------------------------------------------------------------ 6. validation


def test_validation_counts_the_words_that_are_not_residues():
    p, n = P61B, 5
    M = matrix("rand3000x2000", p)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        rows = ctx.rows(blz.V)
        clean = residues(rows, n, p, seed=51)
        assert ctx.set_block_device(blz.V, to_dev(clean, 3)[0], validate=True) == 0
        assert np.array_equal(ctx.get_block(blz.V), flat(clean))
        dirty = clean.copy()
        dirty[17, 2] = p
        dirty[rows - 1, n - 1] = (1 << 64) - 1
        view, _ = to_dev(dirty, 3)
        with pytest.raises(blz.BlzError) as e:
            ctx.set_block_device(blz.V, view, validate=True)
        assert e.value.code == blz.EINVAL and "2 words" in str(e.value), str(e.value)
        assert np.array_equal(ctx.get_block(blz.V), flat(dirty))       # the block holds the words as given
        assert ctx.set_block_device(blz.V, view) is None                # validate=False: the caller's contract, OK
        assert ctx.set_block_device(blz.V, view, validate=False) is None
    with blz.Context(P16, 8) as ctx:                    # 4-byte words, 16-byte lanes impossible: the same count
        ctx.set_matrix(matrix("quirks40x30", P16))
        dirty = residues(40, 8, P16, seed=52)
        dirty[0, 0], dirty[39, 7] = P16, (1 << 64) - 1
        with pytest.raises(blz.BlzError) as e:
            ctx.set_block_device(blz.V, to_dev(dirty)[0], validate=True)
        assert e.value.code == blz.EINVAL and "2 words" in str(e.value)


# ------------------------------------------------------------------------------------------ 7. refusals


def raw_apply(ctx, x, ldx, y, ldy, transpose=0):
    return blz.lib().blz_apply_device(ctx.h, C.c_int(transpose), C.c_void_p(x), C.c_int64(ldx), C.c_void_p(y), C.c_int64(ldy), None)


def refused(rc, *words):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL, (rc, msg)
    for w in words:
        assert w in msg, msg
    return msg


def test_refusals_launch_nothing():
    p, n = P61, 8
    M = matrix("rand3000x2000", p)
    L = blz.lib()
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    with blz.Context(p, n) as ctx:
        none = torch.zeros((3000, n), dtype=torch.int64, device="cuda:0")
        refused(raw_apply(ctx, none.data_ptr(), n, none.data_ptr(), n), "no matrix")
        refused(L.blz_set_block_device(ctx.h, 0, C.c_void_p(none.data_ptr()), C.c_int64(n), None, None), "no matrix")
        refused(L.blz_get_block_device(ctx.h, 0, C.c_void_p(none.data_ptr()), C.c_int64(n), None), "no matrix")
        refused(L.blz_apply_rows(ctx.h, 0, None, None), "no matrix")
        ctx.set_matrix(M)
        v0 = residues(3000, n, p, seed=61)
        ctx.set_block(blz.V, flat(v0))
        x, _ = to_dev(residues(2000, n, p, seed=62))
        x = x.contiguous()
        y = torch.full((3000, n), -1, dtype=torch.int64, device="cuda:0")
        # a host address
        host = np.zeros((3000, n), dtype=np.uint64)
        refused(raw_apply(ctx, host.ctypes.data, n, y.data_ptr(), n), " x ", "not device memory")
        refused(raw_apply(ctx, x.data_ptr(), n, host.ctypes.data, n), " y ", "not device memory")
        refused(L.blz_set_block_device(ctx.h, 0, C.c_void_p(host.ctypes.data), C.c_int64(n), None, None), "dev", "not device memory")
        refused(L.blz_get_block_device(ctx.h, 0, C.c_void_p(host.ctypes.data), C.c_int64(n), None), "dev", "not device memory")
        refused(raw_apply(ctx, 0, n, y.data_ptr(), n), "x is NULL")
        # one row short: an allocation of exactly rows - 1 rows, passed with the full row count
        ld = 512
        short = C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t(2999 * ld * 8)) == 0
        try:
            refused(L.blz_set_block_device(ctx.h, 0, short, C.c_int64(ld), None, None), "dev", "allocation ends")
            refused(L.blz_get_block_device(ctx.h, 0, short, C.c_int64(ld), None), "dev", "allocation ends")
            refused(raw_apply(ctx, x.data_ptr(), n, short.value, ld), " y ", "allocation ends")
            refused(raw_apply(ctx, short.value, ld, x.data_ptr(), n, transpose=1), " x ", "allocation ends")
        finally:
            assert hip.hipFree(short) == 0
        # ld < n
        refused(raw_apply(ctx, x.data_ptr(), n - 1, y.data_ptr(), n), " x ", "less than n")
        refused(raw_apply(ctx, x.data_ptr(), n, y.data_ptr(), 0), " y ", "less than n")
        refused(L.blz_set_block_device(ctx.h, 0, C.c_void_p(y.data_ptr()), C.c_int64(n - 1), None, None), "less than n")
        with pytest.raises(ValueError):
            ctx.apply(False, x[:, :n - 1])
        # x and y overlap
        both = torch.zeros((3000 + 2000, n), dtype=torch.int64, device="cuda:0")
        refused(raw_apply(ctx, both.data_ptr(), n, both.data_ptr() + 1999 * n * 8, n), "overlap")
        refused(raw_apply(ctx, both.data_ptr(), n, both.data_ptr(), n), "overlap")
        assert raw_apply(ctx, both.data_ptr(), n, both.data_ptr() + 2000 * n * 8, n) == blz.OK     # (back to back is fine)
        # a block number of 4
        with pytest.raises(blz.BlzError) as e:
            ctx.set_block_device(4, y)
        assert e.value.code == blz.EINVAL and "block 4" in str(e.value)
        with pytest.raises(blz.BlzError) as e:
            ctx.get_block_device(4, out=y)
        assert e.value.code == blz.EINVAL and "block 4" in str(e.value)
        refused(L.blz_get_block_device(ctx.h, -1, C.c_void_p(y.data_ptr()), C.c_int64(n), None), "block -1")
        # nothing above ran: y untouched, V as it was
        torch.cuda.synchronize()
        assert (to_host(y) == np.uint64((1 << 64) - 1)).all()
        assert np.array_equal(ctx.get_block(blz.V), flat(v0))


def test_a_capturing_stream_is_refused():
    p, n = P61, 8
    M = matrix("rand3000x2000", p)
    L = blz.lib()
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        x = to_dev(residues(2000, n, p, seed=71))[0].contiguous()
        y = torch.full((3000, n), -1, dtype=torch.int64, device="cuda:0")
        ctx.apply(False, x, out=y.clone())              # everything lazy is in place
        s = torch.cuda.Stream(device="cuda:0")
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rcs = [L.blz_apply_device(ctx.h, 0, C.c_void_p(x.data_ptr()), C.c_int64(n), C.c_void_p(y.data_ptr()), C.c_int64(n), h),
                   L.blz_set_block_device(ctx.h, 1, C.c_void_p(x.data_ptr()), C.c_int64(n), h, None),
                   L.blz_get_block_device(ctx.h, 0, C.c_void_p(y.data_ptr()), C.c_int64(n), h)]
            msg = L.blz_last_error().decode()
            x.add_(0)                                   # (a graph of one node, not an empty one)
        assert rcs == [blz.EINVAL] * 3 and "capturing" in msg, (rcs, msg)
        torch.cuda.synchronize()
        assert (to_host(y) == np.uint64((1 << 64) - 1)).all()


def test_several_ranks_are_refused(monkeypatch):
    p, n = P61, 4
    M = matrix("rand3000x2000", p)
    L = blz.lib()
    t = torch.zeros((3000, n), dtype=torch.int64, device="cuda:0")
    grp = blz.LoopGroup(2)
    ctxs = [blz.Context(p, n) for _ in range(2)]
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_loopback(grp, r)
        for c in ctxs:
            refused(raw_apply(c, t.data_ptr(), n, t.data_ptr(), n), "single rank")
            refused(L.blz_set_block_device(c.h, 0, C.c_void_p(t.data_ptr()), C.c_int64(n), None, None), "single rank")
            refused(L.blz_get_block_device(c.h, 0, C.c_void_p(t.data_ptr()), C.c_int64(n), None), "single rank")
    finally:
        for c in ctxs:
            c.close()
        grp.close()
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")           # read when the communicator is attached: one rank, collectives forced on
    one = blz.LoopGroup(1)
    ctx = blz.Context(p, n)
    try:
        ctx.comm_init_loopback(one, 0)
        ctx.set_matrix(M, False, 0, 1)
        for call in (lambda: ctx.apply(False, t[:2000]), lambda: ctx.set_block_device(blz.V, t),
                     lambda: ctx.get_block_device(blz.V, out=t)):
            with pytest.raises(blz.BlzError) as e:
                call()
            assert e.value.code == blz.EINVAL and "single rank" in str(e.value) and "BLZ_FORCE_COMM" in str(e.value)
        assert ctx.apply_rows(False) == (2000, 3000)    # (not a data call)
    finally:
        ctx.close()
        one.close()
