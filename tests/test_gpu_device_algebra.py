"""Device block algebra on the GPU: C = X^T Y (blz_dot_device, Context.dot) and Z = sum X_t A_t (blz_combine_device,
Context.combine) mod p on caller-owned torch tensors, against

  - exact integers: numpy `object` arithmetic on Python ints, and the CPU oracle's block_dot (pinned to the reference's vectors);
  - closed forms where the sums are largest and a big-int reference would be slow: (p-1)^2 = 1, permutations, c - c = 0;
  - blz_iterate on a twin context: the reference's iteration rebuilt from apply, dot and combine, word for word;
  - an undisturbed twin for "the solve is left alone".

Every comparison is equality of u64 words.  Tensors are int64 views of the u64 words where torch has to compute on them (same
bits), torch.uint64 where the library allocates.

The reducer ladder -- the Barrett primes of 33 ... 60 bits, the two primes either side of 2^32, the widths 2 ... 63 this file
leaves out, and blocks long enough that an accumulator passes ModP::chunk -- is tests/test_gpu_device_exact.py.
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
P2, P3, P16, P31 = 2, 3, 65537, (1 << 31) - 1
P61, P61B, P62 = (1 << 61) - 1, (1 << 61) - 31, (1 << 62) - 57
PRIMES = (P2, P3, P16, P31, P61, P61B, P62)
PIDS = ("p2", "p3", "p16", "p31", "p61", "p61b", "p62")
SENTINEL = 0xDEADBEEFCAFEF00D
BIG = 200003
_R = {}


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


def residues(rows, n, p, seed):
    """random residues with 0 and p - 1 in every column (as tests/test_gpu_device_blocks.py); made once, never changed"""
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
    """a random n x n matrix of residues with 0 and p - 1 planted"""
    rng = np.random.default_rng([seed, n, 7])
    a = rng.integers(0, p, size=(n, n), dtype=np.uint64)
    a[rng.integers(0, n), rng.integers(0, n)] = 0
    a[rng.integers(0, n), rng.integers(0, n)] = p - 1
    return a


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


def obj(a):
    return np.asarray(a).astype(object)


def padding_intact(base, n):
    return (to_host(base)[:, n:] == SENTINEL).all()


def sentinel_square(n):
    return torch.from_numpy(np.full((n, n), SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")


def one_base_two_strides(rows, n, p, word=np.uint64):
    """rows * 2n random residues, once as a block of stride n and once, from the SAME pointer, as one of stride 2n: two
    blocks, not one.  (the two views, the words of each on the host); word: np.uint64, or np.uint32 for the 32-bit calls.
    tests/test_gpu_device_fused.py and tests/test_gpu_device_w32.py take it from here."""
    host = np.random.default_rng([11, rows, n]).integers(0, p, size=rows * 2 * n, dtype=word)
    base = torch.from_numpy(host.view(np.int64 if word == np.uint64 else np.int32)).to("cuda:0")
    near, far = base[:rows * n].view(rows, n), base.view(rows, 2 * n)[:, :n]
    assert near.data_ptr() == far.data_ptr() and near.stride(0) == n and far.stride(0) == 2 * n
    return near, far, host[:rows * n].reshape(rows, n), host.reshape(rows, 2 * n)[:, :n]


# ------------------------------------------------------------------------------------------ 1. dot against exact integers


@pytest.mark.parametrize("n", (1, 3, 5, 8, 16, 64))
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_dot_against_exact_integers(p, n):
    with blz.Context(p, n) as ctx:                      # no matrix: the rows are the caller's
        for rows in (0, 1, 2, 63, 257, 1000):
            X, Y = residues(rows, n, p, 1), residues(rows, n, p, 2)
            want = orc.block_dot(rows, flat(Y), flat(X), n, p)[0].reshape(n, n)
            gram = orc.block_dot(rows, flat(X), flat(X), n, p)[1].reshape(n, n)
            if 0 < rows <= 257 and n <= 16:             # Python integers
                assert np.array_equal(want, np.array((obj(X).T @ obj(Y)) % p, dtype=np.uint64).reshape(n, n))
                assert np.array_equal(gram, np.array((obj(X).T @ obj(X)) % p, dtype=np.uint64).reshape(n, n))
            if rows == 0:
                assert not want.any() and not gram.any()
            for padx, pady in ((0, 0), (3, 3), (2, 2), (0, 3)):     # strides n, n + 3 (8-byte lanes), n + 2, and mixed
                (xv, xb), (yv, yb) = to_dev(X, padx), to_dev(Y, pady)
                c = ctx.dot(xv, yv)
                assert c.dtype == torch.uint64 and tuple(c.shape) == (n, n) and c.is_cuda
                assert np.array_equal(to_host(c), want), (rows, padx, pady)
                out = sentinel_square(n)                # the caller's out, every word of it written (zeros at rows = 0)
                assert ctx.dot(xv, yv, out=out) is out
                assert np.array_equal(to_host(out), want), (rows, padx, pady, "out")
                assert np.array_equal(to_host(ctx.dot(xv, xv)), gram), (rows, padx, "x is y")
                assert padding_intact(xb, n) and padding_intact(yb, n)
                assert np.array_equal(to_host(xv), X) and np.array_equal(to_host(yv), Y)
            fl = torch.from_numpy(flat(X).copy().view(np.int64)).to("cuda:0")       # the flat layout of a block
            assert np.array_equal(to_host(ctx.dot(fl, to_dev(Y)[0])), want)
        if n in (3, 8) and p in (P16, P62):             # x and y the same pointer at strides n and 2n: NOT "x is y"
            for rows in (37, 300):                      # one partial tile; several workgroups
                xv, yv, X, Y = one_base_two_strides(rows, n, p)
                want = np.array((obj(X).T @ obj(Y)) % p, dtype=np.uint64).reshape(n, n)      # Python integers
                assert np.array_equal(to_host(ctx.dot(xv, yv)), want), (rows, "one pointer, two strides")
                assert np.array_equal(to_host(ctx.dot(yv, xv)), want.T), (rows, "one pointer, two strides, swapped")


# ------------------------------------------------------------------------------------------ 2. dot at scale


@pytest.mark.parametrize("n", (1, 8, 64))
@pytest.mark.parametrize("p", (P61, P62, P16), ids=("p61", "p62", "p16"))
def test_dot_where_the_sums_are_largest(p, n):
    """200 003 rows: more tiles than workgroups at n = 8 and n = 64, every product (p-1)^2 = 1 mod p"""
    with blz.Context(p, n) as ctx:
        x = torch.full((BIG, n), p - 1, dtype=torch.int64, device="cuda:0")
        y = torch.full((BIG, n + 3), p - 1, dtype=torch.int64, device="cuda:0")[:, :n]
        want = np.full((n, n), BIG % p, dtype=np.uint64)
        assert np.array_equal(to_host(ctx.dot(x, y)), want)
        assert np.array_equal(to_host(ctx.dot(x, x)), want)
        assert np.array_equal(to_host(ctx.dot(y, y)), want)
        if n == 8:                                      # random residues against the oracle
            X, Y = residues(BIG, n, p, 3), residues(BIG, n, p, 4)
            want = orc.block_dot(BIG, flat(Y), flat(X), n, p)[0].reshape(n, n)
            assert np.array_equal(to_host(ctx.dot(to_dev(X)[0], to_dev(Y, 3)[0])), want)


# ------------------------------------------------------------------------------------------ 3. combine against exact integers


def combine_ref(blocks, coeffs, p, n):
    rows = blocks[0].shape[0]
    z = np.zeros((rows, n), dtype=object)
    for X, A in zip(blocks, coeffs):
        z = z + obj(X) @ obj(A)
    return np.array(z % p, dtype=np.uint64).reshape(rows, n)


def combine_cases(ctx, p, n, rows):
    pads = (0, 3, 2, 1)                                 # mixed strides per term
    for nterms in (1, 2, 3, 4):
        Xs = [residues(rows, n, p, 10 + t) for t in range(nterms)]
        As = [coefficient(n, p, 20 + t) for t in range(nterms)]
        want = combine_ref(Xs, As, p, n)
        devs = [to_dev(X, pads[t]) for t, X in enumerate(Xs)]
        # the coefficients as a tensor, a numpy array and a nested list of Python integers
        coef = [torch.from_numpy(A.view(np.int64)).to("cuda:0") if t % 3 == 0 else A if t % 3 == 1 else A.tolist()
                for t, A in enumerate(As)]
        terms = [(devs[t][0], coef[t]) for t in range(nterms)]
        z = ctx.combine(terms)
        assert z.dtype == torch.uint64 and tuple(z.shape) == (rows, n)
        assert np.array_equal(to_host(z), want), (rows, nterms)
        out, base = to_dev(np.full((rows, n), SENTINEL, dtype=np.uint64), 3)        # the caller's strided out
        assert ctx.combine(terms, out=out) is out
        assert np.array_equal(to_host(out), want) and padding_intact(base, n)
        for t in range(nterms):                         # the inputs and their padding as they were
            assert np.array_equal(to_host(devs[t][0]), Xs[t]) and padding_intact(devs[t][1], n)
        # the in-place form: out is the first block (its own stride, its padding untouched)
        assert ctx.combine(terms, out=devs[0][0]) is devs[0][0]
        assert np.array_equal(to_host(devs[0][0]), want), (rows, nterms, "in place")
        assert padding_intact(devs[0][1], n)
        # the same block given as two terms, into a new block and in place
        if nterms >= 2:
            xv, xb = to_dev(Xs[0], 3)
            twice = [(xv, As[0]), (xv, As[1])] + [(devs[t][0], As[t]) for t in range(2, nterms)]
            want2 = combine_ref([Xs[0], Xs[0]] + Xs[2:], As, p, n)
            assert np.array_equal(to_host(ctx.combine(twice)), want2), (rows, nterms, "one block twice")
            assert ctx.combine(twice, out=xv) is xv
            assert np.array_equal(to_host(xv), want2) and padding_intact(xb, n), (rows, nterms, "one block twice, in place")


@pytest.mark.parametrize("n", (1, 3, 8, 16))
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine_against_exact_integers(p, n):
    with blz.Context(p, n) as ctx:
        for rows in (0, 1, 63, 257):
            combine_cases(ctx, p, n, rows)


@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_combine_against_exact_integers_at_n64(p):
    with blz.Context(p, 64) as ctx:                     # four coefficient matrices: 128 KB of LDS
        combine_cases(ctx, p, 64, 70)


# ------------------------------------------------------------------------------------------ 4. combine at scale


@pytest.mark.parametrize("n", (8, 64))
@pytest.mark.parametrize("p", (P61, P62, P16), ids=("p61", "p62", "p16"))
def test_combine_at_scale(p, n):
    dev = "cuda:0"
    with blz.Context(p, n) as ctx:
        # (a) every word and every coefficient p - 1: every product is 1, every word of Z is nterms * n
        x = torch.full((BIG, n), p - 1, dtype=torch.int64, device=dev)
        a = torch.full((n, n), p - 1, dtype=torch.int64, device=dev)
        for nterms in (1, 4):
            z = ctx.combine([(x, a)] * nterms)
            assert (to_host(z) == np.uint64((nterms * n) % p)).all(), nterms
        # (b) a permutation matrix: Z is X with its columns permuted
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        X = torch.randint(0, p, (BIG, n + 2), dtype=torch.int64, device=dev, generator=g)[:, :n]
        perm = np.random.default_rng(6).permutation(n)
        A = np.zeros((n, n), dtype=np.uint64)
        A[perm, np.arange(n)] = 1                       # Z[r, j] = X[r, perm[j]]
        z = ctx.combine([(X, A)])
        assert torch.equal(z.view(torch.int64), X[:, torch.from_numpy(perm).to(dev)])
        # (c) c * X + (p - c) * X = 0, also in place
        c = int(np.random.default_rng(7).integers(1, p))
        eye = np.eye(n, dtype=object)
        Ac, Bc = np.array(eye * c, dtype=np.uint64), np.array(eye * (p - c), dtype=np.uint64)
        z = ctx.combine([(X, Ac), (X, Bc)])
        assert not z.view(torch.int64).any()
        keep = X.clone()
        one = ctx.combine([(X, Ac)])                    # (and c * X alone is not zero)
        assert one.view(torch.int64).any()
        assert ctx.combine([(X, Ac), (X, Bc)], out=X) is X
        assert not X.any()
        assert keep.any()


# ------------------------------------------------------------------------------------------ 5. the iteration, rebuilt


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ((8, P61), (3, P16), (16, P61B)), ids=("n8p61", "n3p16", "n16p61b"))
def test_the_iteration_rebuilt_from_the_device_calls(n, p, right, monkeypatch):
    """sequential/lanczos_modp.c:635-656 out of apply, dot and combine on tensors, against blz_iterate on a twin"""
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    M = blz.Matrix.load(path("rand300x200"), p)
    eye = np.eye(n, dtype=object)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M, right)                        # never iterates
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v = to_dev(twin.get_block(blz.V).reshape(rows, n))[0].contiguous()
        pb = torch.zeros_like(v)
        assert not twin.get_block(blz.P).any()
        for step in range(6):
            assert twin.iterate(1)[:2] == (1, False)
            tmp = ctx.apply(not right, v)
            Av = ctx.apply(right, tmp)
            vtAv, vtAAv = to_host(ctx.dot(v, Av)).reshape(-1), to_host(ctx.dot(Av, Av)).reshape(-1)
            assert np.array_equal(vtAv, twin.get_small(blz.VTAV)), step
            assert np.array_equal(vtAAv, twin.get_small(blz.VTAAV)), step
            npiv, winv, d = orc.semi_inverse(vtAv, n, p)
            assert npiv > 0
            W, A1, A2 = obj(winv).reshape(n, n), obj(vtAv).reshape(n, n), obj(vtAAv).reshape(n, n)
            nz = np.array([int(x) != 0 for x in d])
            D = np.diag(nz.astype(int)).astype(object)
            spliced = np.where(nz[None, :], A2, A1)
            c = (-(W @ spliced)) % p
            vtAvd = (-(A1 @ D)) % p
            v2 = ctx.combine([(Av, D.tolist()), (v, ((eye - D) + c) % p), (pb, vtAvd)])
            p2 = ctx.combine([(pb, (eye - D).tolist()), (v, W)])
            v, pb = v2, p2
            assert np.array_equal(to_host(v).reshape(-1), twin.get_block(blz.V)), step
            assert np.array_equal(to_host(pb).reshape(-1), twin.get_block(blz.P)), step
        assert ctx.iterations == 0 and twin.iterations == 6


# ------------------------------------------------------------------------------------------ 6. the solve is not disturbed


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(s, t) for s, t in zip(a, b))


def foreign_calls(ctx, p, n):
    """a dot and a combine on tensors that have nothing to do with the context's matrix; both checked"""
    X, Y, A, B = residues(777, n, p, 31), residues(777, n, p, 32), coefficient(n, p, 33), coefficient(n, p, 34)
    assert np.array_equal(to_host(ctx.dot(to_dev(X, 3)[0], to_dev(Y)[0])).reshape(-1), orc.block_dot(777, flat(Y), flat(X), n, p)[0])
    xv = to_dev(X)[0]
    ctx.combine([(xv, A), (to_dev(Y, 3)[0], B)], out=xv)
    assert np.array_equal(to_host(xv), combine_ref([X, Y], [A, B], p, n))


def test_dot_and_combine_leave_the_solve_alone(monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")        # p implicit while the iteration runs
    p, n = P61, 8
    M = blz.Matrix.load(path("rand3000x2000"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        for c in (ctx, twin):
            c.set_matrix(M)
            c.init_v()
            assert c.iterate(3)[:2] == (3, False)
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        foreign_calls(ctx, p, n)                        # while p is implicit: the flag and the count do not move
        assert ctx.p_implicit == 1 and ctx.iterations == 3
        before = state(ctx)
        assert same(before, state(twin))
        foreign_calls(ctx, p, n)
        assert same(before, state(ctx))
        trajectory = {id(ctx): [], id(twin): []}
        stopped = False
        while not stopped:                              # on to the stop, both calls between the batches
            stopped = ctx.iterate(16)[1]
            assert twin.iterate(16)[1] == stopped
            foreign_calls(ctx, p, n)
            for c in (ctx, twin):
                trajectory[id(c)].append((c.get_small(blz.VTAV), c.get_small(blz.D), c.iterations))
        assert ctx.iterations == twin.iterations > 3
        assert all(same(a[:2], b[:2]) and a[2] == b[2] for a, b in zip(trajectory[id(ctx)], trajectory[id(twin)]))
        assert same(state(ctx), state(twin))
        assert ctx.final_check() == twin.final_check()
        foreign_calls(ctx, p, n)                        # past the stop every kernel of the solve is a no-op; these are not
        assert same(state(ctx), state(twin))
    with blz.Context(p, n) as bare:                     # and a context with no matrix set
        foreign_calls(bare, p, n)
        foreign_calls(bare, p, n)


# ------------------------------------------------------------------------------------------ 7. stream order


def test_dot_is_ordered_on_the_callers_stream():
    p, n, rows = P61, 8, 3000
    a, b, Y = residues(rows, n, p, 41), residues(rows, n, p, 42), residues(rows, n, p, 43)
    x_host = np.array((obj(a) + obj(b)) % p, dtype=np.uint64)
    want = (obj(orc.block_dot(rows, flat(Y), flat(x_host), n, p)[0]) + 1) % p
    with blz.Context(p, n) as ctx:
        ta, tb, ty = to_dev(a)[0].contiguous(), to_dev(b)[0].contiguous(), to_dev(Y)[0].contiguous()
        ctx.dot(ta, ty)                                 # (scratch and events are in place: nothing synchronous is left)
        big = torch.rand(2048, 2048, device="cuda:0")
        out = sentinel_square(n)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            for _ in range(20):                         # a few milliseconds of work ahead of x on this stream
                big = torch.nn.functional.normalize(big @ big)
            x = torch.remainder(ta + tb + (big[0, 0] > 2).to(torch.int64), p)      # (a + b) mod p, behind the products above
            c = ctx.dot(x, ty, out=out)                 # stream=None: torch's current stream, which is s
            z = torch.remainder(c + 1, p)               # consumed at once
            got = z.cpu().numpy().view(np.uint64)       # the only synchronisation: this copy, on s
    assert np.array_equal(got.reshape(-1), np.array(want, dtype=np.uint64))


# ------------------------------------------------------------------------------------------ 8. refusals


def raw_dot(ctx, rows, x, ldx, y, ldy, c, stream=None):
    return blz.lib().blz_dot_device(ctx.h, C.c_int64(rows), C.c_void_p(x), C.c_int64(ldx), C.c_void_p(y), C.c_int64(ldy),
                                    C.c_void_p(c), stream)


def raw_combine(ctx, rows, xs, lds, cs, z, ldz, nterms=None, stream=None):
    k = len(xs)
    return blz.lib().blz_combine_device(ctx.h, C.c_int64(rows), C.c_int(k if nterms is None else nterms), (C.c_void_p * k)(*xs),
                                        (C.c_int64 * k)(*lds), (C.c_void_p * k)(*cs), C.c_void_p(z), C.c_int64(ldz), stream)


def refused(rc, *words):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL, (rc, msg)
    for w in words:
        assert w in msg, msg
    return msg


def test_refusals_launch_nothing(monkeypatch):
    p, n, rows = P61, 8, 114
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    with blz.Context(p, n) as ctx:
        x = to_dev(residues(rows, n, p, 61))[0].contiguous()
        y = to_dev(residues(rows, n, p, 62))[0].contiguous()
        a = torch.from_numpy(coefficient(n, p, 63).view(np.int64)).to("cuda:0")
        c = sentinel_square(n)
        z = torch.from_numpy(np.full((rows, n), SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")
        x0, y0, a0 = to_host(x).copy(), to_host(y).copy(), to_host(a).copy()
        X, Y, A, Cc, Z = (t.data_ptr() for t in (x, y, a, c, z))
        assert raw_dot(ctx, rows, X, n, Y, n, sentinel_square(n).data_ptr()) == blz.OK     # (the calls below are well formed but for one thing)
        assert raw_combine(ctx, rows, [X, Y], [n, n], [A, A], z.clone().data_ptr(), n) == blz.OK
        # a host address for each argument in turn
        hb, hs = np.zeros((rows, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
        refused(raw_dot(ctx, rows, hb.ctypes.data, n, Y, n, Cc), " x ", "not device memory")
        refused(raw_dot(ctx, rows, X, n, hb.ctypes.data, n, Cc), " y ", "not device memory")
        refused(raw_dot(ctx, rows, X, n, Y, n, hs.ctypes.data), " c ", "not device memory")
        refused(raw_combine(ctx, rows, [hb.ctypes.data, Y], [n, n], [A, A], Z, n), "x[0]", "not device memory")
        refused(raw_combine(ctx, rows, [X, hb.ctypes.data], [n, n], [A, A], Z, n), "x[1]", "not device memory")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [hs.ctypes.data, A], Z, n), "a[0]", "not device memory")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, hs.ctypes.data], Z, n), "a[1]", "not device memory")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, A], hb.ctypes.data, n), " z ", "not device memory")
        # a NULL entry
        refused(raw_dot(ctx, rows, 0, n, Y, n, Cc), "x is NULL")
        refused(raw_dot(ctx, rows, X, n, Y, n, 0), "c is NULL")
        refused(raw_combine(ctx, rows, [X, 0], [n, n], [A, A], Z, n), "x[1] is NULL")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, 0], Z, n), "a[1] is NULL")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, A], 0, n), "z is NULL")
        # one word short: 114 rows at a stride of 9 words are 1025 words; the allocation has 1024
        ld = 9
        assert ((rows - 1) * ld + n) * 8 == 8192 + 8
        short, sq = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t(8192)) == 0
        assert hip.hipMalloc(C.byref(sq), C.c_size_t(n * n * 8 - 8)) == 0
        try:
            refused(raw_dot(ctx, rows, short.value, ld, Y, n, Cc), " x ", "allocation ends")
            refused(raw_dot(ctx, rows, X, n, short.value, ld, Cc), " y ", "allocation ends")
            refused(raw_dot(ctx, rows, X, n, Y, n, sq.value), " c ", "allocation ends")
            refused(raw_combine(ctx, rows, [X, short.value], [n, ld], [A, A], Z, n), "x[1]", "allocation ends")
            refused(raw_combine(ctx, rows, [X, Y], [n, n], [sq.value, A], Z, n), "a[0]", "allocation ends")
            refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, A], short.value, ld), " z ", "allocation ends")
            assert raw_dot(ctx, rows - 1, short.value, ld, Y, n, sentinel_square(n).data_ptr()) == blz.OK      # (one row fewer fits)
        finally:
            torch.cuda.synchronize()
            assert hip.hipFree(short) == 0 and hip.hipFree(sq) == 0
        # ld < n
        refused(raw_dot(ctx, rows, X, n - 1, Y, n, Cc), " x ", "less than n")
        refused(raw_dot(ctx, rows, X, n, Y, 0, Cc), " y ", "less than n")
        refused(raw_combine(ctx, rows, [X, Y], [n, n - 1], [A, A], Z, n), "x[1]", "less than n")
        refused(raw_combine(ctx, rows, [X, Y], [n, n], [A, A], Z, n - 1), " z ", "less than n")
        with pytest.raises(ValueError):
            ctx.dot(x[:, :n - 1], y)
        # overlaps
        both = torch.from_numpy(np.full((2 * rows, n), SENTINEL, dtype=np.uint64).view(np.int64)).to("cuda:0")
        Bp = both.data_ptr()
        refused(raw_combine(ctx, rows, [Bp, Y], [n, n], [A, A], Bp + 8 * n, n), "z overlaps x[0]")          # one row further on
        refused(raw_combine(ctx, rows // 2, [X, Bp], [n, n], [A, A], Bp, 2 * n), "z overlaps x[1]")        # the pointer, another stride
        refused(raw_combine(ctx, n, [X, Y], [n, n], [A, Bp + 8], Bp, n), "z overlaps a[1]")
        refused(raw_combine(ctx, n, [X, Y], [n, n], [Bp, A], Bp, n), "z overlaps a[0]")
        refused(raw_dot(ctx, rows, Bp, n, Y, n, Bp + 8 * n * (rows - 1)), "c overlaps x")
        refused(raw_dot(ctx, rows, X, n, Bp, n, Bp), "c overlaps y")
        # the number of terms, the number of rows
        refused(raw_combine(ctx, rows, [X], [n], [A], Z, n, nterms=0), "nterms = 0")
        refused(raw_combine(ctx, rows, [X] * 5, [n] * 5, [A] * 5, Z, n), "nterms = 5")
        refused(raw_dot(ctx, -1, X, n, Y, n, Cc), "rows = -1")
        refused(raw_combine(ctx, -1, [X], [n], [A], Z, n), "rows = -1")
        for bad in ([], [(x, a)] * 5):
            with pytest.raises(ValueError):
                ctx.combine(bad)
        # a capturing stream
        s = torch.cuda.Stream(device="cuda:0")
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rcs = [raw_dot(ctx, rows, X, n, Y, n, Cc, h)]
            msgs = [blz.lib().blz_last_error().decode()]
            rcs.append(raw_combine(ctx, rows, [X, Y], [n, n], [A, A], Z, n, stream=h))
            msgs.append(blz.lib().blz_last_error().decode())
            x.add_(0)                                   # (a graph of one node, not an empty one)
        assert rcs == [blz.EINVAL] * 2 and all("capturing" in m for m in msgs), (rcs, msgs)
        # nothing above ran: the outputs hold the sentinel, the inputs are what they were
        torch.cuda.synchronize()
        for t in (c, z, both):
            assert (to_host(t) == np.uint64(SENTINEL)).all()
        assert np.array_equal(to_host(x), x0) and np.array_equal(to_host(y), y0) and np.array_equal(to_host(a), a0)
    # a context with the collectives forced on
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")           # read when the communicator is attached
    one = blz.LoopGroup(1)
    ctx = blz.Context(p, n)
    try:
        ctx.comm_init_loopback(one, 0)
        for call in (lambda: ctx.dot(x, y, out=c), lambda: ctx.combine([(x, a)], out=z)):
            with pytest.raises(blz.BlzError) as e:
                call()
            assert e.value.code == blz.EINVAL and "single rank" in str(e.value) and "BLZ_FORCE_COMM" in str(e.value)
    finally:
        ctx.close()
        one.close()
    torch.cuda.synchronize()
    assert (to_host(c) == np.uint64(SENTINEL)).all() and (to_host(z) == np.uint64(SENTINEL)).all()


def test_several_ranks_are_refused():
    p, n = P61, 4
    t = torch.zeros((100, n), dtype=torch.int64, device="cuda:0")
    a = torch.zeros((n, n), dtype=torch.int64, device="cuda:0")
    grp = blz.LoopGroup(2)
    ctxs = [blz.Context(p, n) for _ in range(2)]
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_loopback(grp, r)
        for c in ctxs:
            refused(raw_dot(c, 100, t.data_ptr(), n, t.data_ptr(), n, a.data_ptr()), "single rank")
            refused(raw_combine(c, 100, [t.data_ptr()], [n], [a.data_ptr()], t.data_ptr(), n), "single rank")
    finally:
        for c in ctxs:
            c.close()
        grp.close()
