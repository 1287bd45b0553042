"""32-bit device blocks on the GPU: the eight ...32 calls (csrc/blz_devw32.hip) on torch.int32 / torch.uint32 tensors, against

  - exact integers (numpy `object` arithmetic on Python ints, the CPU oracle's block_dot) and closed forms at scale;
  - the 64-bit namesake on the same residues widened, word for word;
  - set_block + spmv + get_block for the calls that go through the solver's slabs;
  - the reference's own trajectories (tests/golden/traj_*.npz), every step to the stop: vhash, vtAv, vtAAv, winv, d, npiv,
    final_v and final_tmp -- and blz_iterate on a twin context;
  - an undisturbed twin for "the solve is left alone".

Every comparison is equality of words.  The layouts (strides, offsets into the tensor) and the row counts are the case list of
tests/device_w32_ref.py, which tests/test_host_device_w32.py shows to reach every form of every kernel.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import blz
import device_w32_ref as ref
import oracle as orc
from test_gpu_device_algebra import one_base_two_strides

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
PRIMES, PIDS, WIDTHS = ref.PRIMES, ref.PIDS, ref.WIDTHS
P16, P30, P31, P32 = 65537, (1 << 30) - 35, (1 << 31) - 1, (1 << 32) - 5
S32 = 0xCAFEF00D                                        # what every word outside a block holds
S64 = 0xDEADBEEFCAFEF00D
BIG = 200003
_R = {}


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


def obj(a):
    return np.asarray(a).astype(object)


def flat64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def residues(rows, n, p, seed):
    """random u32 residues with 0 and p - 1 planted (at p = 2^32 - 5 and 2^31 - 1 most words are >= 2^30); made once"""
    key = (rows, n, p, seed)
    if key not in _R:
        rng = np.random.default_rng([seed, rows, n])
        w = rng.integers(0, p, size=(rows, n), dtype=np.uint64).astype(np.uint32)
        if rows:
            w[rng.integers(0, rows, 3)] = 0
            w[rng.integers(0, rows, 3)] = p - 1
        w.setflags(write=False)
        _R[key] = w
    return _R[key]


def coefficient(n, p, seed):
    """a random n x n matrix of u64 residues with 0 and p - 1 planted"""
    rng = np.random.default_rng([seed, n, 7])
    a = rng.integers(0, p, size=(n, n), dtype=np.uint64)
    a[rng.integers(0, n), rng.integers(0, n)] = 0
    a[rng.integers(0, n), rng.integers(0, n)] = p - 1
    return a


class Blk:
    """a block of u32 words on the device: `off` words into its tensor, row stride n + pad, every other word S32"""

    def __init__(self, words, pad=0, off=0, unsigned=False):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self.rows, self.n = words.shape
        self.ld, self.off = self.n + pad, off
        host = np.full(off + self.rows * self.ld + 1, S32, dtype=np.uint32)
        host[off:off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.n] = words
        self.base = torch.from_numpy(host.view(np.int32)).to(DEV)
        v = self.base[off:off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.n]
        self.t = v.view(torch.uint32) if unsigned else v
        assert self.rows == 0 or self.t.data_ptr() % 16 == (4 * off) % 16

    def words(self):
        return self.all()[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.n].copy()

    def all(self):
        return self.base.cpu().numpy().view(np.uint32)

    def rest_intact(self):
        """every word that is not the block's still holds the sentinel"""
        a = self.all().copy()
        a[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.n] = S32
        return bool((a == S32).all())


def blank(rows, n, pad=0, off=0, unsigned=False):
    return Blk(np.full((rows, n), S32, dtype=np.uint32), pad, off, unsigned)


def up64(a, pad=0):
    """u64 words on the device as an int64 view of row stride n + pad"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    base = np.full((a.shape[0], a.shape[1] + pad), S64, dtype=np.uint64)
    base[:, :a.shape[1]] = a
    return torch.from_numpy(base.view(np.int64)).to(DEV)[:, :a.shape[1]]


def host64(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def host32(t):
    return t.view(torch.int32).contiguous().cpu().numpy().view(np.uint32)


def sentinel64(*shape):
    return torch.from_numpy(np.full(shape, S64, dtype=np.uint64).view(np.int64)).to(DEV)


def gram_ref(X, Y, p, n):
    return np.array((obj(X).T @ obj(Y)) % p, dtype=np.uint64).reshape(n, n)


def combine_ref(blocks, coeffs, p, n):
    rows = blocks[0].shape[0]
    z = np.zeros((rows, n), dtype=object)
    for X, A in zip(blocks, coeffs):
        if A is not None:
            z = z + obj(X) @ obj(A)
    return np.array(z % p, dtype=np.uint64).reshape(rows, n)


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------ 1. dot32


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_dot32_against_exact_integers_and_the_64_bit_call(p, n):
    with blz.Context(p, n) as ctx:
        assert ctx.word_bytes == 4
        for rows in ref.dot_rows(n)[0]:
            X, Y = residues(rows, n, p, 1), residues(rows, n, p, 2)
            want = orc.block_dot(rows, flat64(Y), flat64(X), n, p)[0].reshape(n, n)
            gram = orc.block_dot(rows, flat64(X), flat64(X), n, p)[1].reshape(n, n)
            if 0 < rows <= 63 and n <= 16:              # Python integers
                assert np.array_equal(want, gram_ref(X, Y, p, n)) and np.array_equal(gram, gram_ref(X, X, p, n))
            if rows == 0:
                assert not want.any() and not gram.any()
            assert np.array_equal(host64(ctx.dot(up64(X), up64(Y, 3))), want)          # the namesake on the widened blocks
            assert np.array_equal(host64(ctx.dot(up64(X), up64(X))), gram)
            for k, (px, ox, py, oy) in enumerate(ref.DOT_LAYOUTS):
                x, y = Blk(X, px, ox, unsigned=k % 2 == 1), Blk(Y, py, oy, unsigned=k % 3 == 1)
                c = ctx.dot32(x.t, y.t)
                assert c.dtype == torch.uint64 and tuple(c.shape) == (n, n) and c.is_cuda
                assert np.array_equal(host64(c), want), (rows, k)
                out = sentinel64(n, n)                  # the caller's out, every word of it written (zeros at rows = 0)
                assert ctx.dot32(x.t, y.t, out=out) is out
                assert np.array_equal(host64(out), want), (rows, k, "out")
                assert np.array_equal(host64(ctx.dot32(x.t, x.t)), gram), (rows, k, "x is y")
                assert x.rest_intact() and y.rest_intact()
                assert np.array_equal(x.words(), X) and np.array_equal(y.words(), Y)
        fl = torch.from_numpy(X.reshape(-1).copy().view(np.int32)).to(DEV)             # the flat layout of a block
        assert np.array_equal(host64(ctx.dot32(fl, Blk(Y).t)), want)


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", (P16, P32), ids=("p16", "p32"))
def test_dot32_with_two_tiles_for_every_workgroup(p, n):
    """more than twice as many tiles as workgroups and a ragged last one: the prefetch of the next tile, the grid stride"""
    rows = ref.dot_rows(n, num_cu())[1]
    X, Y = residues(rows, n, p, 3), residues(rows, n, p, 4)
    with blz.Context(p, n) as ctx:
        want = orc.block_dot(rows, flat64(Y), flat64(X), n, p)[0].reshape(n, n)
        gram = orc.block_dot(rows, flat64(X), flat64(X), n, p)[1].reshape(n, n)
        x, y = Blk(X), Blk(Y, 4 if n % 4 == 0 else 1)
        assert np.array_equal(host64(ctx.dot32(x.t, y.t)), want)
        assert np.array_equal(host64(ctx.dot32(x.t, x.t)), gram)
        c = host64(ctx.dot_pair32(x.t, y.t, y.t))
        assert np.array_equal(c[0], want)
        assert np.array_equal(c[1], orc.block_dot(rows, flat64(Y), flat64(Y), n, p)[1].reshape(n, n))


# ------------------------------------------------------------------------------------------ 2. the largest sums


@pytest.mark.parametrize("n", (1, 8, 64))
def test_dot32_where_the_sums_are_largest(n):
    """every word p - 1 at p = 2^32 - 5 over 200 003 rows: a sum of (p-1)^2 passes 2^81, and (p-1)^2 = 1 mod p"""
    p = P32
    assert BIG * (p - 1) ** 2 > 1 << 81
    with blz.Context(p, n) as ctx:
        x = torch.full((BIG, n), -6, dtype=torch.int32, device=DEV)                    # 0xFFFFFFFA = p - 1, negative as int32
        y = torch.full((BIG, n + 3), p - 1, dtype=torch.int64, device=DEV).to(torch.int32)[:, :n]
        assert int(host32(x)[0, 0]) == p - 1 and int(host32(y)[5, 0]) == p - 1
        want = np.full((n, n), BIG % p, dtype=np.uint64)
        assert np.array_equal(host64(ctx.dot32(x, y)), want)
        assert np.array_equal(host64(ctx.dot32(x, x)), want)
        assert np.array_equal(host64(ctx.dot32(y, y.view(torch.uint32))), want)
        c = host64(ctx.dot_pair32(x, y, y))
        assert np.array_equal(c[0], want) and np.array_equal(c[1], want)
        wide = torch.full((BIG, n), p - 1, dtype=torch.int64, device=DEV)
        assert np.array_equal(host64(ctx.dot(wide, wide)), want)


# ------------------------------------------------------------------------------------------ 3. combine32


def combine32_cases(ctx, p, n, rows, exact):
    for nterms in (1, 2, 3, 4):
        Xs = [residues(rows, n, p, 10 + t) for t in range(nterms)]
        As = [coefficient(n, p, 20 + t) for t in range(nterms)]
        want64 = host64(ctx.combine([(up64(X, t), A) for t, (X, A) in enumerate(zip(Xs, As))]))    # the namesake, widened
        assert want64.max(initial=0) < 1 << 32
        want = want64.astype(np.uint32)
        if exact:
            assert np.array_equal(want64, combine_ref(Xs, As, p, n))
        for k, lay in enumerate(ref.COMBINE_LAYOUTS):
            tag = (rows, nterms, k)

            def fresh():
                return [Blk(X, *lay[t], unsigned=(t + k) % 2 == 1) for t, X in enumerate(Xs)]
            devs = fresh()
            coef = [up64(A) if t % 3 == 0 else A if t % 3 == 1 else A.tolist() for t, A in enumerate(As)]
            terms = [(devs[t].t, coef[t]) for t in range(nterms)]
            z = ctx.combine32(terms)
            assert z.dtype == devs[0].t.dtype and tuple(z.shape) == (rows, n), tag
            assert np.array_equal(host32(z), want), tag
            out = blank(rows, n, *ref.COMBINE_OUT[k])   # the caller's strided out
            assert ctx.combine32(terms, out=out.t) is out.t
            assert np.array_equal(out.words(), want) and out.rest_intact(), tag
            for t in range(nterms):                     # the inputs and everything around them as they were
                assert np.array_equal(devs[t].words(), Xs[t]) and devs[t].rest_intact(), tag
            for t in range(nterms):                     # in place on each term in turn
                devs = fresh()
                terms = [(devs[q].t, As[q]) for q in range(nterms)]
                assert ctx.combine32(terms, out=devs[t].t) is devs[t].t
                assert np.array_equal(devs[t].words(), want) and devs[t].rest_intact(), tag + ("in place", t)
                for q in range(nterms):
                    assert q == t or np.array_equal(devs[q].words(), Xs[q])
        if nterms >= 2 and rows:                        # one block given as two terms, into a new block and in place
            x = Blk(Xs[0], 3)
            twice = [(x.t, As[0]), (x.t, As[1])] + [(up32(Xs[t]), As[t]) for t in range(2, nterms)]
            want2 = host64(ctx.combine([(up64(Xs[0]), As[0]), (up64(Xs[0]), As[1])] +
                                       [(up64(Xs[t]), As[t]) for t in range(2, nterms)])).astype(np.uint32)
            assert np.array_equal(host32(ctx.combine32(twice)), want2)
            ctx.combine32(twice, out=x.t)
            assert np.array_equal(x.words(), want2) and x.rest_intact()


def up32(words):
    return Blk(words).t


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine32_against_exact_integers_and_the_64_bit_call(p, n):
    with blz.Context(p, n) as ctx:
        for rows in ((0, 1, 63, 257) if n <= 16 else (0, 1, 70)):
            combine32_cases(ctx, p, n, rows, exact=rows * n * n <= 70000)


def test_combine32_with_no_rows_touches_nothing():
    p, n = P31, 8
    with blz.Context(p, n) as ctx:
        x, out = Blk(np.zeros((0, n), dtype=np.uint32)), blank(5, n, 3, 1)
        z = ctx.combine32([(x.t, coefficient(n, p, 1))])
        assert tuple(z.shape) == (0, n)
        a = up64(coefficient(n, p, 1))
        rc = blz.lib().blz_combine_device32(ctx.h, C.c_int64(0), C.c_int(1), (C.c_void_p * 1)(out.t.data_ptr()),
                                            (C.c_int64 * 1)(out.ld), (C.c_void_p * 1)(a.data_ptr()),
                                            C.c_void_p(out.t.data_ptr()), C.c_int64(out.ld), None)
        assert rc == blz.OK
        torch.cuda.synchronize()
        assert (out.all() == S32).all()


# ------------------------------------------------------------------------------------------ 4. dot_pair32 and combine_pair32

ALIASES = ref.ALIASES                                   # which of x0, x1, y are one block


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_dot_pair32_in_every_aliasing_pattern(p, n):
    tr = ref.tile_rows(n)
    with blz.Context(p, n) as ctx:
        for rows in (0, 1, 63, tr + 1):
            W = {ch: residues(rows, n, p, 5 + i) for i, ch in enumerate("abc")}
            for pat in ALIASES:
                w64 = {ch: up64(W[ch], i) for i, ch in enumerate("abc")}
                want = host64(ctx.dot_pair(w64[pat[0]], w64[pat[1]], w64[pat[2]]))     # the namesake, widened
                if 0 < rows <= 63 and n <= 16:
                    assert np.array_equal(want[0], gram_ref(W[pat[0]], W[pat[2]], p, n))
                    assert np.array_equal(want[1], gram_ref(W[pat[1]], W[pat[2]], p, n))
                for k, (px, ox, py, oy) in enumerate(ref.DOT_LAYOUTS[::2] if rows != 63 else ref.DOT_LAYOUTS):
                    lay = ref.pair_layout(px, ox, py, oy)
                    d = {ch: Blk(W[ch], *lay[ch], unsigned=(k + i) % 2 == 1) for i, ch in enumerate("abc")}
                    c = ctx.dot_pair32(d[pat[0]].t, d[pat[1]].t, d[pat[2]].t)
                    assert c.dtype == torch.uint64 and tuple(c.shape) == (2, n, n)
                    assert np.array_equal(host64(c), want), (rows, pat, k)
                    out = sentinel64(2, n, n)
                    assert ctx.dot_pair32(d[pat[0]].t, d[pat[1]].t, d[pat[2]].t, out=out) is out
                    assert np.array_equal(host64(out), want), (rows, pat, k, "out")
                    for ch in "abc":
                        assert d[ch].rest_intact() and np.array_equal(d[ch].words(), W[ch])
        # one pointer at two strides (n and 2n) is two blocks: dot32(x, y), and dot_pair32 with x0 = y one block, x1 another
        if n in (3, 8) and p == P16:
            for rows in (37, 300):                      # one partial tile; several workgroups
                near, far, N, F = one_base_two_strides(rows, n, p, np.uint32)
                assert np.array_equal(host64(ctx.dot32(near, far)), gram_ref(N, F, p, n)), (rows, "one pointer, two strides")
                got = host64(ctx.dot_pair32(near, far, near))
                assert np.array_equal(got[0], gram_ref(N, N, p, n)), (rows, "one pointer, two strides", 0)
                assert np.array_equal(got[1], gram_ref(F, N, p, n)), (rows, "one pointer, two strides", 1)


MASKS = {1: [((1, 1),)],                                # the mask list of tests/test_gpu_device_fused.py
         2: [((1, 0), (0, 1)), ((1, 1), (0, 1))],
         3: [((1, 0), (1, 1), (1, 1))],
         4: [((1, 1), (0, 1), (1, 0), (1, 1)), ((1, 1), (1, 1), (1, 1), (1, 1))]}


def combine_pair32_case(ctx, p, n, rows, masks, k, exact):
    nterms, lay = len(masks), ref.COMBINE_LAYOUTS[k]
    Xs = [residues(rows, n, p, 10 + t) for t in range(nterms)]
    A0 = [coefficient(n, p, 20 + t) if m[0] else None for t, m in enumerate(masks)]
    A1 = [coefficient(n, p, 30 + t) if m[1] else None for t, m in enumerate(masks)]
    tag = (rows, masks, k)
    w64 = [up64(X) for X in Xs]
    w0, w1 = (host64(z) for z in ctx.combine_pair([(w64[t], A0[t], A1[t]) for t in range(nterms)]))     # the namesake, widened
    if exact:
        assert np.array_equal(w0, combine_ref(Xs, A0, p, n)) and np.array_equal(w1, combine_ref(Xs, A1, p, n)), tag
    w0, w1 = w0.astype(np.uint32), w1.astype(np.uint32)

    def fresh():
        return [Blk(X, *lay[t], unsigned=(t + k) % 2 == 0) for t, X in enumerate(Xs)]

    def terms_of(devs, kind=0):
        conv = lambda A, t: None if A is None else (up64(A) if (t + kind) % 3 == 0 else A if (t + kind) % 3 == 1 else A.tolist())
        return [(devs[t].t, conv(A0[t], t), conv(A1[t], t)) for t in range(nterms)]
    devs = fresh()
    z0, z1 = ctx.combine_pair32(terms_of(devs))
    assert z0.dtype == z1.dtype == devs[0].t.dtype and tuple(z0.shape) == tuple(z1.shape) == (rows, n)
    assert np.array_equal(host32(z0), w0) and np.array_equal(host32(z1), w1), tag
    o0, o1 = blank(rows, n, *ref.COMBINE_OUT[k]), blank(rows, n, 2, 1)
    got = ctx.combine_pair32(terms_of(devs, 1), out=(o0.t, o1.t))
    assert got[0] is o0.t and got[1] is o1.t
    assert np.array_equal(o0.words(), w0) and np.array_equal(o1.words(), w1), tag
    assert o0.rest_intact() and o1.rest_intact()
    for t in range(nterms):
        assert np.array_equal(devs[t].words(), Xs[t]) and devs[t].rest_intact()
    devs, z1 = fresh(), blank(rows, n)                  # z0 in place on the last term, z1 fresh
    ctx.combine_pair32(terms_of(devs, 2), out=(devs[-1].t, z1.t))
    assert np.array_equal(devs[-1].words(), w0) and np.array_equal(z1.words(), w1), tag + ("z0 in place",)
    assert devs[-1].rest_intact()
    devs, z0 = fresh(), blank(rows, n)                  # z1 in place on the first term, z0 fresh
    ctx.combine_pair32(terms_of(devs), out=(z0.t, devs[0].t))
    assert np.array_equal(z0.words(), w0) and np.array_equal(devs[0].words(), w1), tag + ("z1 in place",)
    if nterms >= 2:                                     # both in place on different terms: v and p of a Lanczos step
        devs = fresh()
        ctx.combine_pair32(terms_of(devs, 1), out=(devs[-2].t, devs[-1].t))
        assert np.array_equal(devs[-2].words(), w0) and np.array_equal(devs[-1].words(), w1), tag + ("both in place",)
        assert devs[-2].rest_intact() and devs[-1].rest_intact()
        for t in range(nterms - 2):
            assert np.array_equal(devs[t].words(), Xs[t])


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine_pair32_against_exact_integers_and_the_64_bit_call(p, n):
    with blz.Context(p, n) as ctx:
        for rows in ((0, 1, 63, 257) if n <= 16 else (0, 70)):
            for nterms in (1, 2, 3, 4):
                for masks in MASKS[nterms]:
                    for k in range(len(ref.COMBINE_LAYOUTS)):
                        if k not in (2, 4) and rows not in (63, 70):
                            continue                    # the uniform layouts at one row count, the mixed ones everywhere
                        combine_pair32_case(ctx, p, n, rows, masks, k, exact=rows * n * n <= 70000 and k == 2)


# ------------------------------------------------------------------------------------------ 5. set / get / apply32 / apply_pair32


def slab_cases(make, p, n, right):
    """the four calls that go through the solver's slabs against set_block + spmv + get_block on a context made the same way"""
    with make() as ctx, make() as hostctx:
        vr, tr_ = ctx.apply_rows(not right)             # rows of V (and AV, P) and of TMP
        assert (vr, tr_) == (ctx.rows(blz.V), ctx.rows(blz.TMP))
        V = residues(vr, n, p, 71)
        V64 = V.astype(np.uint64)
        hostctx.set_block(blz.V, V64.reshape(-1))
        hostctx.spmv(not right, blz.V, blz.TMP)
        hostctx.spmv(right, blz.TMP, blz.AV)
        T = hostctx.get_block(blz.TMP).reshape(tr_, n)
        AV = hostctx.get_block(blz.AV).reshape(vr, n)
        assert T.max(initial=0) < 1 << 32 and AV.max(initial=0) < 1 << 32
        T, AV = T.astype(np.uint32), AV.astype(np.uint32)
        for k, (pad, off) in enumerate(ref.IO_LAYOUTS):
            uns = k % 2 == 1
            x = Blk(V, pad, off, uns)
            # set32 -> host get; host set -> get32; set32 -> get32: the same words
            assert ctx.set_block_device32(blz.V, x.t, validate=True) == 0
            assert np.array_equal(ctx.get_block(blz.V), V64.reshape(-1)), (k, "set32, host get")
            out = blank(vr, n, pad, off, uns)
            assert ctx.get_block_device32(blz.V, out=out.t) is out.t
            assert np.array_equal(out.words(), V) and out.rest_intact(), (k, "get32")
            ctx.set_block(blz.AV, AV.astype(np.uint64).reshape(-1))
            got = ctx.get_block_device32(blz.AV)
            assert got.dtype == torch.uint32 and np.array_equal(host32(got), AV), (k, "host set, get32")
            # apply32 both ways
            y = blank(tr_, n, pad, off, uns)
            assert ctx.apply32(not right, x.t, out=y.t) is y.t
            assert np.array_equal(y.words(), T) and y.rest_intact(), (k, "apply32")
            z = ctx.apply32(right, y.t)
            assert z.dtype == y.t.dtype and np.array_equal(host32(z), AV), (k, "apply32 back")
            # apply_pair32: without the intermediate, with it, into the caller's blocks, in place
            assert np.array_equal(host32(ctx.apply_pair32(not right, x.t)), AV), (k, "pair")
            z, mid = ctx.apply_pair32(not right, x.t, mid=True)
            assert np.array_equal(host32(z), AV) and np.array_equal(host32(mid), T), (k, "pair, mid")
            o, m = blank(vr, n, 2, 2), blank(tr_, n, 3, 1)
            got = ctx.apply_pair32(not right, x.t, out=o.t, mid=m.t)
            assert got[0] is o.t and got[1] is m.t
            assert np.array_equal(o.words(), AV) and np.array_equal(m.words(), T) and o.rest_intact() and m.rest_intact()
            assert np.array_equal(x.words(), V) and x.rest_intact()
            assert ctx.apply_pair32(not right, x.t, out=x.t) is x.t
            assert np.array_equal(x.words(), AV) and x.rest_intact(), (k, "pair in place")
        # the 64-bit calls on the widened block give the same words
        assert np.array_equal(host64(ctx.apply(not right, up64(V64))), T.astype(np.uint64))
        # bad counts the words that are not below p, a planted 0xFFFFFFFF among them
        planted = V.copy()
        planted[0, 0] = 0xFFFFFFFF
        planted[vr - 1, n - 1] = 0xFFFFFFFF
        count = 2
        if p < (1 << 32) - 1:
            planted[vr // 2, 0] = p
            count = 3
        with pytest.raises(blz.BlzError) as err:
            ctx.set_block_device32(blz.V, Blk(planted, 1, 1).t, validate=True)
        assert err.value.code == blz.EINVAL and f"{count} words" in str(err.value)
        assert ctx.iterations == 0


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("name, p, n", (("rand300x200", P32, 8), ("rand300x200", P16, 8), ("quirks40x30", P30, 5),
                                         ("quirks40x30", P31, 5)), ids=("rand-p32n8", "rand-p16n8", "quirks-p30n5", "quirks-p31n5"))
def test_the_slab_calls_against_set_block_spmv_get_block(name, p, n, right):
    M = blz.Matrix.load(path(name), p)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix(M, right)
        return ctx
    slab_cases(make, p, n, right)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
def test_the_slab_calls_on_a_bordered_context(right):
    p, n, k = P30, 4, 3
    M = blz.Matrix.load(path("rand300x200"), p)
    b = residues(M.nrows if right else M.ncols, k, p, seed=k).astype(np.uint64)

    def make():
        ctx = blz.Context(p, n)
        ctx.set_matrix_rhs_block(M, b, right)
        assert ctx.rhs_count == k
        return ctx
    slab_cases(make, p, n, right)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
def test_the_slab_calls_in_signed_mode(right):
    p, n = P31, 2
    M = blz.Matrix.load_signed(path("graph200x600"))

    def make():
        ctx = blz.Context(p, n)
        ctx.set_values_signed()
        ctx.set_matrix(M, right)
        assert ctx.values_signed() and ctx.word_bytes == 4      # (4-byte words: the entries are canonicalised at upload)
        return ctx
    slab_cases(make, p, n, right)


# ------------------------------------------------------------------------------------------ 6. the iteration from four 32-bit calls


def step32(ctx, right, v, pb):
    """sequential/lanczos_modp.c:635-656 in four 32-bit calls and ortho_coeffs, v and p updated in place"""
    Av = ctx.apply_pair32(not right, v)
    c = ctx.dot_pair32(v, Av, Av)                       # vtAv, vtAAv
    coef, npiv = ctx.ortho_coeffs(c[0], c[1])
    ctx.combine_pair32([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                        (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))
    return c, coef, npiv


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint64).tobytes()).hexdigest()


@pytest.mark.parametrize("traj", ("traj_r300_p1073741789_n8_left", "traj_r300_p65537_n4_right", "traj_r300_p2147483647_n4_left"))
def test_the_iteration_rebuilt_from_the_32_bit_calls(traj, monkeypatch):
    """Every step of the reference's own run, to its stop and with the stopping step: before step k sha256 of v (widened to
    u64 words) is vhash[k]; the step's vtAv, vtAAv, winv, d and npiv are the reference's; after the last step, which finds
    npiv = 0 and changes nothing, v is final_v and M applied to it is final_tmp.  The same steps against blz_iterate."""
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    g = np.load(os.path.join(GOLDEN, traj + ".npz"))
    p, n, right, stop = int(g["prime"]), int(g["n"]), bool(g["right"]), int(g["stop_after"])
    steps = len(g["npiv"])                              # the whole trajectory: 26, 51 and 51 steps
    assert stop <= 0 and steps == len(g["vhash"]) == int(g["iterations"]) + 1
    assert int(g["npiv"][-1]) == 0 and all(int(x) > 0 for x in g["npiv"][:-1])
    M = blz.Matrix.load(path("rand300x200"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M, right)                        # never iterates
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v0 = twin.get_block(blz.V)
        assert np.array_equal(v0, g["v0"])
        want = []
        for _ in range(steps):
            done, stopped = twin.iterate(1)[:2]
            want.append((done, stopped, twin.get_small(blz.VTAV), twin.get_small(blz.VTAAV), twin.get_small(blz.WINV),
                         twin.get_small(blz.D), twin.get_block(blz.V), twin.get_block(blz.P)))
        assert twin.iterations == int(g["iterations"])
        v = Blk(v0.reshape(rows, n).astype(np.uint32)).t.contiguous()
        pb = torch.zeros((rows, n), dtype=torch.int32, device=DEV)
        got = []
        for _ in range(steps):                          # no tensor is read on the host in here
            before = v.clone()
            c, coef, npiv = step32(ctx, right, v, pb)
            winv, d, npiv2 = ctx.semi_inverse_device(c[0])      # (the 64-bit n x n call serves both families)
            got.append((before, v.clone(), pb.clone(), c, coef, npiv, winv, d, npiv2))
        final_tmp = host32(ctx.apply32(not right, v))
        assert ctx.iterations == 0
        got = [(host32(b), host32(gv), host32(gp)) + tuple(host64(t) for t in rest) for b, gv, gp, *rest in got]
    for k, ((b, gv, gp, c, coef, npiv, winv, d, npiv2), (done, stopped, wA, wAA, wW, wd, wv, wp)) in enumerate(zip(got, want)):
        last = k == steps - 1
        # the reference's own run
        assert sha(b.reshape(-1)) == str(g["vhash"][k]), k
        assert np.array_equal(c[0].reshape(-1), g["vtAv"][k]) and np.array_equal(c[1].reshape(-1), g["vtAAv"][k]), k
        assert np.array_equal(winv.reshape(-1), g["winv"][k]) and np.array_equal(d, g["d"][k]), k
        assert int(npiv[0]) == int(npiv2[0]) == int(g["npiv"][k]) == int(d.sum()), k
        if not last:
            assert np.array_equal(np.diagonal(coef[blz.COEF_V_AV]), g["d"][k]), k
        # blz_iterate on the twin
        assert (done, stopped) == ((0, True) if last else (1, False)), k
        assert np.array_equal(c[0].reshape(-1), wA) and np.array_equal(c[1].reshape(-1), wAA), k
        assert np.array_equal(winv.reshape(-1), wW) and np.array_equal(d, wd), k
        assert np.array_equal(gv.reshape(-1).astype(np.uint64), wv), k
        assert np.array_equal(gp.reshape(-1).astype(np.uint64), wp), k
    # the stopping step changed nothing, and the run ends where the reference's ends
    assert np.array_equal(got[-1][1], got[-1][0])
    assert np.array_equal(got[-1][1].reshape(-1).astype(np.uint64), g["final_v"])
    assert np.array_equal(final_tmp.reshape(-1).astype(np.uint64), g["final_tmp"])


# ------------------------------------------------------------------------------------------ 7. the solve is left alone; stream order


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(s, t) for s, t in zip(a, b))


def foreign_calls(ctx, plain, p, n):
    """the 32-bit calls on tensors that have nothing to do with the solve, interleaved with 64-bit ones; all checked"""
    X, Y, Z = residues(777, n, p, 51), residues(777, n, p, 52), residues(777, n, p, 53)
    A, B = coefficient(n, p, 54), coefficient(n, p, 55)
    x, y, z = Blk(X, 3), Blk(Y), Blk(Z, 2, 2)
    c = host64(ctx.dot_pair32(x.t, y.t, y.t))
    assert np.array_equal(c, host64(ctx.dot_pair(up64(X), up64(Y), up64(Y))))
    assert np.array_equal(host64(ctx.dot32(x.t, z.t)), host64(ctx.dot(up64(X), up64(Z))))
    want = [host64(t).astype(np.uint32) for t in ctx.combine_pair([(up64(X), A, None), (up64(Y), B, A), (up64(Z), A, B)])]
    ctx.combine_pair32([(x.t, A, None), (y.t, B, A), (z.t, A, B)], out=(y.t, z.t))
    assert np.array_equal(y.words(), want[0]) and np.array_equal(z.words(), want[1])
    xr, _ = ctx.apply_rows(False)
    W = residues(xr, n, p, 56)
    got, mid = ctx.apply_pair32(False, Blk(W).t, mid=True)
    m64 = plain.apply(False, up64(W))
    assert np.array_equal(host32(mid), host64(m64).astype(np.uint32))
    assert np.array_equal(host32(got), host64(plain.apply(True, m64)).astype(np.uint32))
    assert np.array_equal(host32(ctx.apply32(False, Blk(W, 1, 1).t)), host32(mid))


def test_the_32_bit_calls_leave_the_solve_alone(monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    p, n = P31, 8
    M = blz.Matrix.load(path("rand3000x2000"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin, blz.Context(p, n) as plain:
        plain.set_matrix(M)
        for c in (ctx, twin):
            c.set_matrix(M)
            c.init_v()
            assert c.iterate(3)[:2] == (3, False)
        implicit = ctx.p_implicit
        foreign_calls(ctx, plain, p, n)
        assert ctx.p_implicit == implicit and ctx.iterations == 3
        before = state(ctx)
        assert same(before, state(twin))
        foreign_calls(ctx, plain, p, n)
        assert same(before, state(ctx))
        stopped = False
        while not stopped:                              # on to the stop, the calls between the batches
            stopped = ctx.iterate(16)[1]
            assert twin.iterate(16)[1] == stopped
            foreign_calls(ctx, plain, p, n)
            assert np.array_equal(ctx.get_small(blz.VTAV), twin.get_small(blz.VTAV)) and ctx.iterations == twin.iterations
        assert ctx.iterations == twin.iterations > 3
        assert same(state(ctx), state(twin))
        assert ctx.final_check() == twin.final_check()


def test_the_32_bit_calls_are_ordered_on_the_callers_stream():
    p, n, rows = P30, 8, 3000
    a, b, Y, Z = (residues(rows, n, p, 41 + k) for k in range(4))
    A, B = coefficient(n, p, 45), coefficient(n, p, 46)
    M = blz.Matrix.load(path("rand3000x2000"), p)
    x_host = np.array((obj(a) + obj(b)) % p, dtype=np.uint64).astype(np.uint32)
    plus1 = lambda t: np.array((obj(t) + 1) % p, dtype=np.uint64)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        assert ctx.apply_rows(False) == (2000, 3000)
        want_c = host64(ctx.dot_pair(up64(x_host), up64(Y), up64(Y)))
        want_z = [host64(t) for t in ctx.combine_pair([(up64(x_host), A, B), (up64(Y), B, None), (up64(Z), None, A)])]
        want_w = host64(ctx.apply(True, ctx.apply(False, up64(x_host[:2000]))))
        ta, tb, ty, tz, tA, tB = up32(a), up32(b), up32(Y), up32(Z), up64(A), up64(B)
        ctx.dot_pair32(ta, ty, ty)                      # (scratch, slabs and events are in place: nothing synchronous is left)
        ctx.apply_pair32(False, ta[:2000].contiguous())
        big = torch.rand(2048, 2048, device=DEV)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            for _ in range(20):                         # a few milliseconds of work ahead of x on this stream
                big = torch.nn.functional.normalize(big @ big)
            x = torch.remainder(ta.to(torch.int64) + tb.to(torch.int64) + (big[0, 0] > 2).to(torch.int64), p).to(torch.int32)
            c = ctx.dot_pair32(x, ty, ty)               # stream=None: torch's current stream, which is s
            z0, z1 = ctx.combine_pair32([(x, tA, tB), (ty, tB, None), (tz, None, tA)])
            w = ctx.apply_pair32(False, x[:2000])
            used = [torch.remainder(t.view(torch.int64) + 1, p) for t in (c, z0.to(torch.int64), z1.to(torch.int64), w.to(torch.int64))]
            got = [t.cpu().numpy().view(np.uint64) for t in used]
    assert np.array_equal(got[0], plus1(want_c).reshape(2, n, n))
    assert np.array_equal(got[1], plus1(want_z[0]).reshape(rows, n)) and np.array_equal(got[2], plus1(want_z[1]).reshape(rows, n))
    assert np.array_equal(got[3], plus1(want_w).reshape(2000, n))


# ------------------------------------------------------------------------------------------ 8. refusals


def vp(x):
    return C.c_void_p(x)


def raw_set(ctx, x, ld, stream=None):
    return blz.lib().blz_set_block_device32(ctx.h, C.c_int(blz.V), vp(x), C.c_int64(ld), stream, None)


def raw_get(ctx, x, ld, stream=None):
    return blz.lib().blz_get_block_device32(ctx.h, C.c_int(blz.V), vp(x), C.c_int64(ld), stream)


def raw_apply(ctx, x, ldx, y, ldy, stream=None):
    return blz.lib().blz_apply_device32(ctx.h, C.c_int(0), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), stream)


def raw_apply2(ctx, x, ldx, y, ldy, z, ldz, stream=None):
    return blz.lib().blz_apply_pair_device32(ctx.h, C.c_int(0), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), vp(z),
                                             C.c_int64(ldz), stream)


def raw_dot(ctx, rows, x, ldx, y, ldy, c, stream=None):
    return blz.lib().blz_dot_device32(ctx.h, C.c_int64(rows), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), vp(c), stream)


def raw_dot2(ctx, rows, x0, ld0, x1, ld1, y, ldy, c, stream=None):
    return blz.lib().blz_dot_pair_device32(ctx.h, C.c_int64(rows), vp(x0), C.c_int64(ld0), vp(x1), C.c_int64(ld1), vp(y),
                                           C.c_int64(ldy), vp(c), stream)


def raw_combine(ctx, rows, xs, lds, a, z, ldz, stream=None):
    k = len(xs)
    return blz.lib().blz_combine_device32(ctx.h, C.c_int64(rows), C.c_int(k), (C.c_void_p * k)(*xs), (C.c_int64 * k)(*lds),
                                          (C.c_void_p * k)(*a), vp(z), C.c_int64(ldz), stream)


def raw_combine2(ctx, rows, xs, lds, a0, a1, z0, ldz0, z1, ldz1, stream=None):
    k = len(xs)
    return blz.lib().blz_combine_pair_device32(ctx.h, C.c_int64(rows), C.c_int(k), (C.c_void_p * k)(*xs), (C.c_int64 * k)(*lds),
                                               (C.c_void_p * k)(*a0), (C.c_void_p * k)(*a1), vp(z0), C.c_int64(ldz0), vp(z1),
                                               C.c_int64(ldz1), stream)


def refused(rc, *parts):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL, (rc, msg)
    for w in parts:
        assert w in msg, msg
    return msg


def all_eight(ctx, X, Y, A, Cc, Z, W, rows, n, stream=None):
    """the eight calls, well formed on a context that takes them; X is read, Y / Z / W / Cc would be written"""
    return (lambda: raw_set(ctx, X, n, stream), lambda: raw_get(ctx, Z, n, stream),
            lambda: raw_apply(ctx, X, n, Z, n, stream), lambda: raw_apply2(ctx, X, n, Z, n, W, n, stream),
            lambda: raw_dot(ctx, rows, X, n, Y, n, Cc, stream), lambda: raw_dot2(ctx, rows, X, n, Y, n, Y, n, Cc, stream),
            lambda: raw_combine(ctx, rows, [X, Y], [n, n], [A, A], Z, n, stream),
            lambda: raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Z, n, W, n, stream))


def test_refusals_launch_nothing(monkeypatch):
    p, n, rows = P31, 8, 114
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    M = blz.Matrix.synth(rows, rows, 4 * rows, 5, p)    # square: every block of the slab calls has `rows` rows
    x, y = Blk(residues(rows, n, p, 61)), Blk(residues(rows, n, p, 62))
    a = up64(coefficient(n, p, 63))
    a0 = host64(a).copy()
    c, z, w, both = sentinel64(2, n, n), blank(rows, n), blank(rows, n), blank(2 * rows, n)
    X, Y, A, Cc, Z, W, Bp = (t.data_ptr() for t in (x.t, y.t, a, c, z.t, w.t, both.t))
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M)
        assert ctx.apply_rows(False) == (rows, rows)
        ok = [blank(rows, n) for _ in range(2)]
        okc = sentinel64(2, n, n)
        for call in all_eight(ctx, X, Y, A, okc.data_ptr(), ok[0].t.data_ptr(), ok[1].t.data_ptr(), rows, n):
            assert call() == blz.OK, blz.lib().blz_last_error().decode()      # (well formed but for one thing below)
        assert raw_apply2(ctx, X, n, 0, 0, ok[1].t.data_ptr(), n) == blz.OK   # y may be NULL
        assert raw_dot(ctx, 0, 0, n, 0, n, okc.data_ptr()) == blz.OK          # no rows: any block pointer
        # a pointer at byte offset 2
        refused(raw_dot(ctx, rows - 1, X + 2, n, Y, n, Cc), " x ", "aligned to 4 bytes")
        refused(raw_dot(ctx, rows - 1, X, n, Y + 2, n, Cc), " y ", "aligned to 4 bytes")
        refused(raw_dot2(ctx, rows - 1, X, n, Y + 2, n, Y, n, Cc), " x1 ", "aligned to 4 bytes")
        refused(raw_combine(ctx, rows - 1, [X + 2], [n], [A], Z, n), "x[0]", "aligned to 4 bytes")
        refused(raw_combine(ctx, rows - 1, [X], [n], [A], Z + 2, n), " z ", "aligned to 4 bytes")
        refused(raw_combine2(ctx, rows - 1, [X], [n], [A], [A], Z, n, W + 2, n), " z1 ", "aligned to 4 bytes")
        refused(raw_set(ctx, Bp + 2, n), " dev ", "aligned to 4 bytes")
        refused(raw_get(ctx, Bp + 2, n), " dev ", "aligned to 4 bytes")
        refused(raw_apply(ctx, X, n, Bp + 2, n), " y ", "aligned to 4 bytes")
        refused(raw_apply2(ctx, X, n, 0, 0, Bp + 2, n), " z ", "aligned to 4 bytes")
        # the coefficients and the results stay 8-byte words
        refused(raw_dot(ctx, rows, X, n, Y, n, Cc + 4), " c ", "aligned to 8 bytes")
        refused(raw_combine(ctx, rows, [X], [n], [A + 4], Z, n), "a[0]", "aligned to 8 bytes")
        # ld < n
        refused(raw_dot(ctx, rows, X, n - 1, Y, n, Cc), " x ", "less than n")
        refused(raw_dot2(ctx, rows, X, n, Y, n, Y, 0, Cc), " y ", "less than n")
        refused(raw_combine(ctx, rows, [X, Y], [n, n - 1], [A, A], Z, n), "x[1]", "less than n")
        refused(raw_combine2(ctx, rows, [X], [n], [A], [A], Z, n - 1, W, n), " z0 ", "less than n")
        refused(raw_set(ctx, X, n - 1), " dev ", "less than n")
        refused(raw_get(ctx, Z, n - 1), " dev ", "less than n")
        refused(raw_apply(ctx, X, n, Z, n - 1), " y ", "less than n")
        refused(raw_apply2(ctx, X, n - 1, 0, 0, Z, n), " x ", "less than n")
        # a host pointer
        hb, hs = np.zeros((rows, n), dtype=np.uint32), np.zeros((2, n, n), dtype=np.uint64)
        H, HS = hb.ctypes.data, hs.ctypes.data
        refused(raw_dot(ctx, rows, H, n, Y, n, Cc), " x ", "not device memory")
        refused(raw_dot(ctx, rows, X, n, Y, n, HS), " c ", "not device memory")
        refused(raw_dot2(ctx, rows, X, n, H, n, Y, n, Cc), " x1 ", "not device memory")
        refused(raw_combine(ctx, rows, [X], [n], [HS], Z, n), "a[0]", "not device memory")
        refused(raw_combine(ctx, rows, [X], [n], [A], H, n), " z ", "not device memory")
        refused(raw_combine2(ctx, rows, [X, H], [n, n], [A, A], [A, A], Z, n, W, n), "x[1]", "not device memory")
        refused(raw_set(ctx, H, n), " dev ", "not device memory")
        refused(raw_get(ctx, H, n), " dev ", "not device memory")
        refused(raw_apply(ctx, H, n, Z, n), " x ", "not device memory")
        refused(raw_apply2(ctx, X, n, H, n, Z, n), " y ", "not device memory")
        # one word short: 114 rows at a stride of 9 words are 1025 words; the allocation has 1024
        ld = 9
        assert ((rows - 1) * ld + n) * 4 == 4096 + 4
        short = C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t(4096)) == 0
        try:
            S = short.value
            refused(raw_dot(ctx, rows, S, ld, Y, n, Cc), " x ", "allocation ends")
            refused(raw_dot2(ctx, rows, X, n, Y, n, S, ld, Cc), " y ", "allocation ends")
            refused(raw_combine(ctx, rows, [X], [n], [A], S, ld), " z ", "allocation ends")
            refused(raw_combine2(ctx, rows, [S], [ld], [A], [A], Z, n, W, n), "x[0]", "allocation ends")
            refused(raw_set(ctx, S, ld), " dev ", "allocation ends")
            refused(raw_get(ctx, S, ld), " dev ", "allocation ends")
            refused(raw_apply(ctx, X, n, S, ld), " y ", "allocation ends")
            refused(raw_apply2(ctx, X, n, 0, 0, S, ld), " z ", "allocation ends")
            assert raw_dot(ctx, rows - 1, S, ld, Y, n, okc.data_ptr()) == blz.OK       # one row less fits
        finally:
            torch.cuda.synchronize()
            assert hip.hipFree(short) == 0
        # a byte offset that leaves 64 bits
        refused(raw_dot(ctx, 1 << 40, X, 1 << 40, Y, n, Cc), " x ", "64-bit")
        # every forbidden overlap (4-byte words: a row of n words is 4 n bytes)
        half = rows // 2
        refused(raw_dot(ctx, n, Cc, n, Y, n, Cc), "c overlaps x")
        refused(raw_dot(ctx, n, X, n, Cc, n, Cc), "c overlaps y")
        refused(raw_dot2(ctx, n, X, n, Cc, n, Y, n, Cc), "c overlaps x1")
        refused(raw_combine(ctx, rows, [Bp, Y], [n, n], [A, A], Bp + 4 * n, n), "z overlaps x[0]")      # a row on
        refused(raw_combine(ctx, half, [Bp, Y], [n, n], [A, A], Bp, 2 * n), "z overlaps x[0]")           # another stride
        refused(raw_combine(ctx, n, [X], [n], [Bp], Bp, n), "z overlaps a[0]")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], Bp, n, Bp + 4 * n * (rows - 1), n), "z0 overlaps z1")
        refused(raw_combine2(ctx, rows, [X, Y], [n, n], [A, A], [A, A], X, n, X, n), "z0 overlaps z1")
        refused(raw_combine2(ctx, half, [X, Bp], [n, n], [A, A], [A, A], Z, n, Bp, 2 * n), "z1 overlaps x[1]")
        refused(raw_apply(ctx, Bp, n, Bp + 4 * n * (rows - 1), n), "x and y overlap")
        refused(raw_apply2(ctx, Bp, n, 0, 0, Bp + 4 * n, n), "z overlaps x")
        refused(raw_apply2(ctx, Bp, n, 0, 0, Bp, n + 1), "z overlaps x")
        refused(raw_apply2(ctx, Bp, n, Bp + 4 * n * (rows - 1), n, W, n), "y overlaps x")
        refused(raw_apply2(ctx, X, n, Bp + 4 * n * (rows - 1), n, Bp, n), "y overlaps z")
        # an int64 tensor passed to a ...32 method, an int32 one to a 64-bit method
        t64 = torch.zeros((rows, n), dtype=torch.int64, device=DEV)
        for call in (lambda: ctx.dot32(t64, y.t), lambda: ctx.dot32(x.t, t64), lambda: ctx.dot_pair32(x.t, t64, y.t),
                     lambda: ctx.combine32([(t64, a)]), lambda: ctx.combine32([(x.t, a)], out=t64),
                     lambda: ctx.combine_pair32([(x.t, a, a)], out=(z.t, t64)), lambda: ctx.set_block_device32(blz.V, t64),
                     lambda: ctx.get_block_device32(blz.V, out=t64), lambda: ctx.apply32(False, t64),
                     lambda: ctx.apply_pair32(False, x.t, out=t64), lambda: ctx.dot(x.t, x.t)):
            with pytest.raises(ValueError) as err:
                call()
            assert "dtype" in str(err.value)
        # a capturing stream
        s = torch.cuda.Stream(device=DEV)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rcs, msgs = [], []
            for call in all_eight(ctx, X, Y, A, Cc, Z, W, rows, n, h):
                rcs.append(call())
                msgs.append(blz.lib().blz_last_error().decode())
            a.add_(0)                                   # (a graph of one node, not an empty one)
        assert rcs == [blz.EINVAL] * 8 and all("capturing" in m for m in msgs), (rcs, msgs)
        # device blocks on ranks switched on
        ctx.device_ranks(True)
        for call in all_eight(ctx, X, Y, A, Cc, Z, W, rows, n):
            refused(call(), "single rank", "blz_set_device_ranks")
        ctx.device_ranks(False)
        assert raw_dot(ctx, rows, X, n, Y, n, okc.data_ptr()) == blz.OK
    # p >= 2^32: the residues do not fit
    for big in ((1 << 32) + 15, (1 << 61) - 1):
        with blz.Context(big, n) as wide:
            assert wide.word_bytes == 8
            wide.set_matrix(blz.Matrix.synth(rows, rows, 4 * rows, 5, big))
            for call in all_eight(wide, X, Y, A, Cc, Z, W, rows, n):
                refused(call(), "residues do not fit 32-bit words")
            with pytest.raises(blz.BlzError) as err:
                wide.dot32(x.t, y.t, out=c[0])
            assert err.value.code == blz.EINVAL and "do not fit" in str(err.value)
    # a loopback group of one with the collectives forced on, and a group of two
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")
    for nranks in (1, 2):
        grp = blz.LoopGroup(nranks)
        ctxs = [blz.Context(p, n) for _ in range(nranks)]
        try:
            for r, cx in enumerate(ctxs):
                cx.comm_init_loopback(grp, r)
            for cx in ctxs:
                for call in all_eight(cx, X, Y, A, Cc, Z, W, rows, n)[4:]:             # (the slab calls would need a matrix)
                    refused(call(), "single rank")
                refused(raw_apply(cx, X, n, Z, n), "single rank")
        finally:
            for cx in ctxs:
                cx.close()
            grp.close()
    # nothing above ran: the outputs hold their sentinel, the inputs are what they were
    torch.cuda.synchronize()
    assert (host64(c) == np.uint64(S64)).all()
    for t in (z, w, both):
        assert (t.all() == S32).all()
    assert np.array_equal(x.words(), residues(rows, n, p, 61)) and np.array_equal(y.words(), residues(rows, n, p, 62))
    assert np.array_equal(host64(a), a0)
    with blz.Context(p, n) as bare:                     # the slab calls need a matrix; the other four do not
        for call in all_eight(bare, X, Y, A, Cc, Z, W, rows, n)[:4]:
            rc = call()
            assert rc == blz.EINVAL and "no matrix" in blz.lib().blz_last_error().decode()
