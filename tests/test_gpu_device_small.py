"""Device small algebra on the GPU: blz_semi_inverse_device (Context.semi_inverse_device), blz_ortho_coeffs_device
(Context.ortho_coeffs) and blz_rref_device (Context.rref) on caller-owned torch tensors, against

  - the reference's own vectors (tests/golden/semi_inverse.npz) and the CPU oracle's semi_inverse, which is pinned to them;
  - a Python-integer restatement of the five coefficient panels and of the elimination (kbasis_ref.py);
  - Context.block_rref and Context.kernel_basis on a twin context that holds the same rows;
  - blz_iterate on a twin context: the iteration rebuilt from apply, dot, ortho_coeffs and combine with nothing read on the
    host inside the loop, from the usual and from a rank-deficient start, and on past the stop;
  - an undisturbed twin for "the solve is left alone".

Every comparison is equality of u64 words.  The reducer ladder -- every reducer class of csrc/modp.h, k_dev_chain at 1024
threads with lg = 5, k_dev_rref with lane groups of 2 and 32 and a reduction past ModP::chunk -- is
tests/test_gpu_device_exact.py.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import blz
import kbasis_ref as kb
import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P2, P3, P16, P31 = 2, 3, 65537, (1 << 31) - 1
P61, P61B, P62 = (1 << 61) - 1, (1 << 61) - 31, (1 << 62) - 57
PRIMES = (P2, P3, P16, P31, P61, P61B, P62)
PIDS = ("p2", "p3", "p16", "p31", "p61", "p61b", "p62")
WIDTHS = (1, 3, 5, 8, 16, 64)
SENTINEL = 0xDEADBEEFCAFEF00D
DEV = "cuda:0"
ITER_CASES = ((8, P61), (3, P16), (16, P61B))           # the grid of the rebuilt-iteration test of test_gpu_device_algebra.py
ITER_IDS = ("n8p61", "n3p16", "n16p61b")
_CACHE = {}


def path(name):
    return os.path.join(GOLDEN, name + ".mtx")


def obj(a):
    return np.asarray(a).astype(object)


def words(a):
    """an array of Python integers (or anything) as u64 words"""
    return np.array(a, dtype=np.uint64)


def flat(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def up(a, shape=None):
    """u64 words to the device (int64 bits), contiguous"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy((a if shape is None else a.reshape(shape)).view(np.int64).copy()).to(DEV)


def to_dev(w, pad=0, fill=SENTINEL):
    """(view of shape (rows, n) with row stride n + pad, the base tensor) on the device"""
    w = np.ascontiguousarray(w, dtype=np.uint64)
    base = np.full((w.shape[0], w.shape[1] + pad), fill, dtype=np.uint64)
    base[:, :w.shape[1]] = w
    tb = torch.from_numpy(base.view(np.int64)).to(DEV)
    return tb[:, :w.shape[1]], tb


def to_host(t):
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)


def sentinel(*shape):
    return torch.from_numpy(np.full(shape, SENTINEL, dtype=np.uint64).view(np.int64)).to(DEV)


def square_inputs(n, p):
    """the n x n inputs of items 2 and 3, made once: random symmetric, B^T B of rank <= n // 2, zero, identity, all p - 1,
    and an independent random vtaav"""
    key = ("sq", n, p)
    if key not in _CACHE:
        rng = np.random.default_rng([n, p % 1000003, 17])
        R = obj(rng.integers(0, p, size=(n, n), dtype=np.uint64))
        B = obj(rng.integers(0, p, size=(n // 2, n), dtype=np.uint64))
        mats = {"symmetric": (R + R.T) % p, "low rank": (B.T @ B) % p if n // 2 else np.zeros((n, n), dtype=object),
                "zero": np.zeros((n, n), dtype=object), "identity": np.eye(n, dtype=object),
                "all p - 1": np.full((n, n), p - 1, dtype=object)}
        other = rng.integers(0, p, size=(n, n), dtype=np.uint64)
        out = {}
        for name, M in mats.items():
            M = words(M).reshape(n, n)
            npiv, winv, d = orc.semi_inverse(flat(M), n, p)
            out[name] = (M, int(npiv), flat(winv).copy(), flat(d).copy())
        _CACHE[key] = (out, other)
    return _CACHE[key]


def panels_ref(vtav, vtaav, winv, d, n, p):
    """the five panels of include/blz.h from the oracle's winv and d, on Python integers"""
    W, A1, A2, eye = obj(winv).reshape(n, n), obj(vtav).reshape(n, n), obj(vtaav).reshape(n, n), np.eye(n, dtype=object)
    nz = np.array([int(x) != 0 for x in d])
    D = np.diag(nz.astype(int)).astype(object)
    S = np.where(nz[None, :], A2, A1)
    return words(np.stack([D % p, ((eye - D) - W @ S) % p, (-(A1 @ D)) % p, (eye - D) % p, W % p]))


# ------------------------------------------------------------------------------------------ 1. the reference's own vectors


def test_semi_inverse_device_against_the_golden_vectors():
    g = np.load(os.path.join(GOLDEN, "semi_inverse.npz"))
    keys = sorted(k[:-2] for k in g.files if k.endswith("_M"))
    assert keys
    for key in keys:
        n, p = int(key.split("_")[0][1:]), int(key.split("_")[1][1:])
        with blz.Context(p, n) as ctx:
            for M, winv, d, npiv in zip(g[key + "_M"], g[key + "_winv"], g[key + "_d"], g[key + "_npiv"]):
                w, dd, k = ctx.semi_inverse_device(up(M, (n, n)))
                assert w.dtype == dd.dtype == k.dtype == torch.uint64
                assert tuple(w.shape) == (n, n) and tuple(dd.shape) == (n,) and tuple(k.shape) == (1,)
                assert int(to_host(k)[0]) == int(npiv), key
                assert np.array_equal(to_host(w).reshape(-1), flat(winv)) and np.array_equal(to_host(dd), flat(d)), key


# ------------------------------------------------------------------------------------------ 2. against the oracle


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_semi_inverse_device_against_the_oracle(p, n):
    cases, _ = square_inputs(n, p)
    assert cases["zero"][1] == 0 and not cases["zero"][2].any() and not cases["zero"][3].any()
    assert cases["identity"][1] == n
    with blz.Context(p, n) as ctx:                      # no matrix
        for name, (M, npiv, winv, d) in cases.items():
            a = up(M)
            w, dd, k = ctx.semi_inverse_device(a)
            assert int(to_host(k)[0]) == npiv, name
            assert np.array_equal(to_host(dd), d), name
            assert np.array_equal(to_host(w).reshape(-1), winv), name
            assert np.array_equal(to_host(a), M), name  # the input as it was


# ------------------------------------------------------------------------------------------ 3. the coefficient panels


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_ortho_coeffs_against_python_integers(p, n):
    cases, other = square_inputs(n, p)
    with blz.Context(p, n) as ctx:
        b = up(other)
        for name, (M, npiv, winv, d) in cases.items():
            want = panels_ref(M, other, winv, d, n, p)
            assert (obj(want) < p).all()
            coef, k = ctx.ortho_coeffs(up(M), b)
            assert coef.dtype == torch.uint64 and tuple(coef.shape) == (5, n, n) and coef.is_contiguous()
            got = to_host(coef)
            assert int(to_host(k)[0]) == npiv, name
            assert (obj(got) < p).all(), name
            assert np.array_equal(got, want), name
            out = sentinel(5, n, n)                     # the caller's out: every word written
            assert ctx.ortho_coeffs(up(M), b, out=out)[0] is out
            assert np.array_equal(to_host(out), want), name
        eye = words(np.eye(n, dtype=object) % p)
        stop = to_host(ctx.ortho_coeffs(up(cases["zero"][0]), b)[0])   # npiv = 0: the step is the identity on v and p
        assert not stop[blz.COEF_V_AV].any() and not stop[blz.COEF_V_P].any() and not stop[blz.COEF_P_V].any()
        assert np.array_equal(stop[blz.COEF_V_V], eye) and np.array_equal(stop[blz.COEF_P_P], eye)


# ------------------------------------------------------------------------------------------ 4.-6. the iteration, host-free


def device_step(ctx, right, v, pb):
    """sequential/lanczos_modp.c:635-656 out of apply, dot, ortho_coeffs and combine: nothing is read on the host"""
    tmp = ctx.apply(not right, v)
    Av = ctx.apply(right, tmp)
    vtAv, vtAAv = ctx.dot(v, Av), ctx.dot(Av, Av)
    coef, npiv = ctx.ortho_coeffs(vtAv, vtAAv)
    v2 = ctx.combine([(Av, coef[blz.COEF_V_AV]), (v, coef[blz.COEF_V_V]), (pb, coef[blz.COEF_V_P])])
    p2 = ctx.combine([(pb, coef[blz.COEF_P_P]), (v, coef[blz.COEF_P_V])])
    return v2, p2, vtAv, vtAAv, coef, npiv


def deficient_start(v0, n):
    """column 1 <- column 0, column 2 <- 0 (nothing at n = 1)"""
    v0 = v0.copy()
    if n >= 2:
        v0[:, 1] = v0[:, 0]
    if n >= 3:
        v0[:, 2] = 0
    return v0


def rebuilt_against_twin(n, p, right, steps, deficient):
    """(per-step records of the device loop, per-step records of the twin); the twin may stop early (tiny p)"""
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
        assert not twin.get_block(blz.P).any()
        want = []
        for _ in range(steps):
            done, stopped = twin.iterate(1)[:2]
            want.append((done, stopped, twin.get_small(blz.VTAV), twin.get_small(blz.VTAAV), twin.get_small(blz.D),
                         twin.get_block(blz.V), twin.get_block(blz.P)))
        v, pb = to_dev(v0)[0].contiguous(), torch.zeros((rows, n), dtype=torch.int64, device=DEV)
        got = []
        for _ in range(steps):                          # no tensor is read on the host in here
            v, pb, vtAv, vtAAv, coef, npiv = device_step(ctx, right, v, pb)
            got.append((v, pb, vtAv, vtAAv, coef, npiv))
        assert ctx.iterations == 0
        return [tuple(to_host(t) for t in rec) for rec in got], want


def compare_steps(got, want, n, expect_running):
    for step, ((v, pb, vtAv, vtAAv, coef, npiv), (done, stopped, wA, wAA, wd, wv, wp)) in enumerate(zip(got, want)):
        if expect_running:
            assert (done, stopped) == (1, False), step
        if done:                                        # (a twin that has stopped keeps the operands of its last real step)
            assert np.array_equal(vtAv.reshape(-1), wA), step
            assert np.array_equal(vtAAv.reshape(-1), wAA), step
            assert np.array_equal(np.diagonal(coef[blz.COEF_V_AV]), wd), step
            assert int(npiv[0]) == int(wd.sum()) > 0, step
        else:
            assert int(npiv[0]) == 0, step
        assert np.array_equal(v.reshape(-1), wv), step
        assert np.array_equal(pb.reshape(-1), wp), step


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_the_iteration_rebuilt_with_nothing_on_the_host(n, p, right, monkeypatch):
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    got, want = rebuilt_against_twin(n, p, right, 6, deficient=False)
    compare_steps(got, want, n, expect_running=True)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_the_iteration_rebuilt_from_a_rank_deficient_start(n, p, right, monkeypatch):
    """column 1 = column 0 and column 2 = 0: d = 1 0 0 1 ... 1 at each of the first eight steps (the CPU oracle says so for
    these six cases), so npiv > 0 and the D-dependent panels differ from the full-rank ones at every step"""
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    got, want = rebuilt_against_twin(n, p, right, 8, deficient=True)
    compare_steps(got, want, n, expect_running=True)
    pattern = np.array([1, 0, 0] + [1] * (n - 3), dtype=np.uint64)
    for step, rec in enumerate(got):
        assert np.array_equal(np.diagonal(rec[4][blz.COEF_V_AV]), pattern), step
        assert int(rec[5][0]) == n - 2, step


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_the_rank_deficient_start_at_every_prime_and_width(p, n):
    """the same start at every reducer class and width (left); at a tiny p the twin may stop early, and the device loop is
    then the identity on v and p"""
    got, want = rebuilt_against_twin(n, p, False, 6, deficient=True)
    compare_steps(got, want, n, expect_running=False)


@pytest.mark.parametrize("right", (False, True), ids=("left", "right"))
@pytest.mark.parametrize("n, p", ITER_CASES, ids=ITER_IDS)
def test_the_loop_runs_past_the_stop_without_a_look(n, p, right, monkeypatch):
    """80 steps, more than the 25, 67 and 13 iterations after which these cases stop: v and p stay what they were at the stop"""
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    M = blz.Matrix.load(path("rand300x200"), p)
    with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
        ctx.set_matrix(M, right)
        twin.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v = to_dev(twin.get_block(blz.V).reshape(rows, n))[0].contiguous()
        pb = torch.zeros_like(v)
        for _ in range(80):
            v, pb, _, _, _, npiv = device_step(ctx, right, v, pb)
        done, stopped = twin.iterate(200)[:2]
        assert stopped and 0 < done < 80
        assert np.array_equal(to_host(v).reshape(-1), twin.get_block(blz.V))
        assert np.array_equal(to_host(pb).reshape(-1), twin.get_block(blz.P))
        assert int(to_host(npiv)[0]) == 0
        assert ctx.iterations == 0 and twin.iterations == done


# ------------------------------------------------------------------------------------------ 7. rref


def ctx_with_rows(p, n, R):
    """a context whose V block has R rows (left kernel of an R x 5 matrix)"""
    c = blz.Context(p, n)
    c.set_matrix(blz.Matrix.synth(R, 5, 2 * R, 1, p), right=False)
    return c


def rref_blocks(rng, p, n, R):
    dense = rng.integers(0, p, size=(R, n), dtype=np.uint64)
    out = {"dense": dense}
    cols = deficient_start(dense, n)                    # a repeated and a zero column
    out["repeated and zero columns"] = cols
    out["repeated rows"] = rng.integers(0, p, size=(3, n), dtype=np.uint64)[rng.integers(0, 3, size=R)]
    if R > n:                                           # the first n rows decide; the others are copies of them
        lead = dense.copy()
        lead[n:] = lead[rng.integers(0, n, size=R - n)]
        out["full rank first, then nothing new"] = lead
        B, _ = kb.random_rref(rng, n // 2, n, p)
        out["planted, half rank"] = kb.planted_block(rng, R, B, n // 2, p)
    out["zero"] = np.zeros((R, n), dtype=np.uint64)
    return out


def info_of(r, piv, n):
    return np.array([r] + list(piv) + [-1] * (n - r), dtype=np.int64)


def check_rref(ctx, X, p, n, E, r, piv, tag):
    Z = words(kb.null_basis(E, r, piv, n, p)).reshape(n, n)
    E = words(E).reshape(n, n)
    for pad in (0, 3):
        xv, xb = to_dev(X, pad)
        e, z, info = ctx.rref(xv)
        assert e.dtype == z.dtype == torch.uint64 and info.dtype == torch.int64
        assert tuple(e.shape) == tuple(z.shape) == (n, n) and tuple(info.shape) == (n + 1,)
        assert np.array_equal(info.cpu().numpy(), info_of(r, piv, n)), (tag, pad)
        assert np.array_equal(to_host(e), E), (tag, pad)
        assert np.array_equal(to_host(z), Z), (tag, pad)
        assert (to_host(xb)[:, n:] == SENTINEL).all() and np.array_equal(to_host(xv), X), (tag, pad)
        assert not to_host(ctx.combine([(e, z)])).any(), (tag, pad)       # e * z = 0
    e, z, info = ctx.rref(to_dev(X)[0], null=False)
    assert z is None and np.array_equal(to_host(e), E) and int(info[0]) == r, tag


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("p", PRIMES, ids=PIDS)
def test_rref_against_block_rref_and_python_integers(p, n):
    rng = np.random.default_rng([p % 1000003, n, 23])
    with blz.Context(p, n) as ctx:                      # no matrix: the rows are the caller's
        check_rref(ctx, np.zeros((0, n), dtype=np.uint64), p, n, np.zeros((n, n), dtype=object), 0, [], "no rows")
        e, z, info = ctx.rref(torch.zeros((0, n), dtype=torch.int64, device=DEV))
        assert not to_host(e).any() and np.array_equal(to_host(z), words(np.eye(n, dtype=object)))
        assert np.array_equal(info.cpu().numpy(), info_of(0, [], n))
        for R in (1, 2, 63, 257, 1000):
            with ctx_with_rows(p, n, R) as twin:
                for name, X in rref_blocks(rng, p, n, R).items():
                    twin.set_block(blz.V, X.reshape(-1))
                    E, r, piv = twin.block_rref(blz.V)
                    if R <= 257 and n <= 16:            # the elimination on Python integers
                        Ek, rk, pk = kb.rref(X.tolist(), p, n)
                        assert (r, piv) == (rk, list(pk)) and np.array_equal(E, words(Ek).reshape(n, n)), (R, name)
                    if name == "dense" and R >= n and p > P16:
                        assert r == n                   # full rank: E = I
                    if name == "full rank first, then nothing new" and p > P16:
                        assert r == n
                    check_rref(ctx, X, p, n, obj(E), r, piv, (R, name))


# ------------------------------------------------------------------------------------------ 8. the kernel basis, rebuilt


@pytest.mark.parametrize("deps, n, right, p", ((1, 8, False, 1073741789), (2, 8, True, P16), (2, 8, False, P61), (3, 4, False, P31)),
                         ids=("d1n8", "d2n8right", "d2n8p61", "d3n4p31"))
def test_the_kernel_basis_rebuilt_on_the_callers_blocks(tmp_path, deps, n, right, p):
    m = kb.planted_kernel_matrix(str(tmp_path / "m.mtx"), 300, 310 if deps == 2 and not right else 300, deps, deps, right=right)
    M = blz.Matrix.load(m, p)
    with blz.Context(p, n) as twin, blz.Context(p, n) as ctx:         # ctx has no matrix: the candidates are tensors
        twin.set_matrix(M, right)
        twin.init_v()
        assert twin.iterate(2000)[1]
        V, T = twin.get_block_device(blz.V), twin.get_block_device(blz.TMP)
        _, Z0, _ = ctx.rref(T)                          # 1. and 2.
        Y = ctx.combine([(V, Z0)])                      # 3.
        _, _, info = ctx.rref(Y, null=False)            # 4.
        info = info.cpu().numpy()
        k, piv = int(info[0]), [int(q) for q in info[1:1 + int(info[0])]]
        basis = to_host(Y)[:, piv]
        z = np.zeros((n, n), dtype=np.uint64)
        z[:, :k] = to_host(Z0)[:, piv]                  # Z0 times the column selection
        wk, wz = twin.kernel_basis()
        assert k == wk == deps
        assert np.array_equal(z, wz)
        got = twin.get_block(blz.V).reshape(-1, n)
        assert np.array_equal(got[:, :k], basis) and not got[:, k:].any()


# ------------------------------------------------------------------------------------------ 9. the solve is not disturbed


def state(ctx):
    return ([ctx.get_block(b) for b in (blz.V, blz.TMP, blz.AV, blz.P)] +
            [ctx.get_small(w) for w in (blz.VTAV, blz.VTAAV, blz.WINV, blz.D)] + [np.array([ctx.iterations])])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(s, t) for s, t in zip(a, b))


def foreign_calls(ctx, p, n):
    """the three calls on tensors that have nothing to do with the context's matrix; all checked"""
    cases, other = square_inputs(n, p)
    for name in ("symmetric", "low rank"):
        M, npiv, winv, d = cases[name]
        w, dd, k = ctx.semi_inverse_device(up(M))
        assert int(to_host(k)[0]) == npiv and np.array_equal(to_host(w).reshape(-1), winv) and np.array_equal(to_host(dd), d)
        coef, k = ctx.ortho_coeffs(up(M), up(other))
        assert int(to_host(k)[0]) == npiv and np.array_equal(to_host(coef), panels_ref(M, other, winv, d, n, p))
    key = ("foreign", n, p)
    if key not in _CACHE:
        X = deficient_start(np.random.default_rng(91).integers(0, p, size=(777, n), dtype=np.uint64), n)
        _CACHE[key] = (X,) + kb.rref(X.tolist(), p, n)
    X, E, r, piv = _CACHE[key]
    e, z, info = ctx.rref(to_dev(X, 3)[0])
    assert np.array_equal(to_host(e), words(E).reshape(n, n)) and np.array_equal(info.cpu().numpy(), info_of(r, piv, n))
    assert np.array_equal(to_host(z), words(kb.null_basis(E, r, piv, n, p)).reshape(n, n))


def test_the_small_algebra_leaves_the_solve_alone(monkeypatch):
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
        assert ctx.block_rref(blz.V)[1] == twin.block_rref(blz.V)[1]     # the solver's own echelon buffers are its own
        foreign_calls(ctx, p, n)
        trajectory = {id(ctx): [], id(twin): []}
        stopped = False
        while not stopped:                              # on to the stop, the calls between the batches
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
        kc, zc = ctx.kernel_basis()
        kt, zt = twin.kernel_basis()
        assert kc == kt and np.array_equal(zc, zt)
    with blz.Context(p, n) as bare:                     # and a context with no matrix set
        foreign_calls(bare, p, n)
        foreign_calls(bare, p, n)


# ------------------------------------------------------------------------------------------ 10. stream order


def test_the_calls_are_ordered_on_the_callers_stream():
    p, n, rows = P61, 8, 3000
    rng = np.random.default_rng(41)
    a, b = (rng.integers(0, p, size=(n, n), dtype=np.uint64) for _ in range(2))
    other = rng.integers(0, p, size=(n, n), dtype=np.uint64)
    xa, xb_ = (deficient_start(rng.integers(0, p, size=(rows, n), dtype=np.uint64), n) for _ in range(2))
    m_host, x_host = words((obj(a) + obj(b)) % p), words((obj(xa) + obj(xb_)) % p)
    npiv, winv, d = orc.semi_inverse(flat(m_host), n, p)
    want_coef = panels_ref(m_host, other, winv, d, n, p)
    E, r, piv = kb.rref(x_host.tolist(), p, n)
    with blz.Context(p, n) as ctx:
        ta, tb, to, txa, txb = up(a), up(b), up(other), up(xa), up(xb_)
        ctx.rref(txa)                                   # (scratch and events are in place: nothing synchronous is left)
        ctx.ortho_coeffs(ta, to)
        big = torch.rand(2048, 2048, device=DEV)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            for _ in range(20):                         # a few milliseconds of work ahead of the operands on this stream
                big = torch.nn.functional.normalize(big @ big)
            late = (big[0, 0] > 2).to(torch.int64)
            m = torch.remainder(ta + tb + late, p)      # (a + b) mod p, behind the products above
            x = torch.remainder(txa + txb + late, p)
            w, dd, k = ctx.semi_inverse_device(m)       # stream=None: torch's current stream, which is s
            coef, k2 = ctx.ortho_coeffs(m, to)
            e, z, info = ctx.rref(x)
            used = [torch.remainder(t.view(torch.int64) + 1, p) for t in (w, coef, e)]     # consumed at once
            got = [t.cpu().numpy() for t in used + [dd.view(torch.int64), k.view(torch.int64), k2.view(torch.int64), info]]
    plus1 = lambda t: words((obj(t) + 1) % p)
    assert np.array_equal(got[0].view(np.uint64).reshape(-1), plus1(flat(winv)))
    assert np.array_equal(got[1].view(np.uint64), plus1(want_coef))
    assert np.array_equal(got[2].view(np.uint64), plus1(words(E).reshape(n, n)))
    assert np.array_equal(got[3].view(np.uint64), flat(d)) and int(got[4][0]) == int(got[5][0]) == npiv
    assert np.array_equal(got[6], info_of(r, piv, n))


# ------------------------------------------------------------------------------------------ 11. refusals


def raw_semi(ctx, a, w, d, k, stream=None):
    return blz.lib().blz_semi_inverse_device(ctx.h, C.c_void_p(a), C.c_void_p(w), C.c_void_p(d), C.c_void_p(k), stream)


def raw_coef(ctx, a, b, cf, k, stream=None):
    return blz.lib().blz_ortho_coeffs_device(ctx.h, C.c_void_p(a), C.c_void_p(b), C.c_void_p(cf), C.c_void_p(k), stream)


def raw_rref(ctx, rows, x, ld, e, z, info, stream=None):
    return blz.lib().blz_rref_device(ctx.h, C.c_int64(rows), C.c_void_p(x), C.c_int64(ld), C.c_void_p(e), C.c_void_p(z),
                                     C.c_void_p(info), stream)


def refused(rc, *parts):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL, (rc, msg)
    for w in parts:
        assert w in msg, msg
    return msg


def test_refusals_launch_nothing(monkeypatch):
    p, n, rows = P61, 8, 114
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    rng = np.random.default_rng(61)
    with blz.Context(p, n) as ctx:
        a, b = up(rng.integers(0, p, size=(n, n), dtype=np.uint64)), up(rng.integers(0, p, size=(n, n), dtype=np.uint64))
        x = up(rng.integers(0, p, size=(rows, n), dtype=np.uint64))
        a0, b0, x0 = to_host(a).copy(), to_host(b).copy(), to_host(x).copy()
        w, d, k, cf, e, z, info = sentinel(n, n), sentinel(n), sentinel(1), sentinel(5, n, n), sentinel(n, n), sentinel(n, n), sentinel(n + 1)
        both = sentinel(2 * rows, n)
        A, B, X, W, D, K, CF, E, Z, I, Bp = (t.data_ptr() for t in (a, b, x, w, d, k, cf, e, z, info, both))
        ok = [sentinel(5, n, n) for _ in range(3)]      # (the calls below are well formed but for one thing)
        assert raw_semi(ctx, A, ok[0].data_ptr(), ok[1].data_ptr(), ok[2].data_ptr()) == blz.OK
        assert raw_semi(ctx, A, ok[0].data_ptr(), ok[1].data_ptr(), 0) == blz.OK               # npiv may be NULL
        assert raw_coef(ctx, A, B, ok[0].data_ptr(), 0) == blz.OK
        assert raw_coef(ctx, A, A, ok[0].data_ptr(), ok[2].data_ptr()) == blz.OK               # inputs may be one matrix
        assert raw_rref(ctx, rows, X, n, ok[0].data_ptr(), 0, ok[1].data_ptr()) == blz.OK      # z may be NULL
        assert raw_rref(ctx, 0, 0, n, ok[0].data_ptr(), ok[2].data_ptr(), ok[1].data_ptr()) == blz.OK      # no rows: any x
        # a host address for each argument in turn
        hs, hb = np.zeros((5, n, n), dtype=np.uint64), np.zeros((rows, n), dtype=np.uint64)
        H = hs.ctypes.data
        refused(raw_semi(ctx, H, W, D, K), " vtav ", "not device memory")
        refused(raw_semi(ctx, A, H, D, K), " winv ", "not device memory")
        refused(raw_semi(ctx, A, W, H, K), " d ", "not device memory")
        refused(raw_semi(ctx, A, W, D, H), " npiv ", "not device memory")
        refused(raw_coef(ctx, H, B, CF, K), " vtav ", "not device memory")
        refused(raw_coef(ctx, A, H, CF, K), " vtaav ", "not device memory")
        refused(raw_coef(ctx, A, B, H, K), " coef ", "not device memory")
        refused(raw_coef(ctx, A, B, CF, H), " npiv ", "not device memory")
        refused(raw_rref(ctx, rows, hb.ctypes.data, n, E, Z, I), " x ", "not device memory")
        refused(raw_rref(ctx, rows, X, n, H, Z, I), " e ", "not device memory")
        refused(raw_rref(ctx, rows, X, n, E, H, I), " z ", "not device memory")
        refused(raw_rref(ctx, rows, X, n, E, Z, H), " info ", "not device memory")
        # a NULL entry
        refused(raw_semi(ctx, 0, W, D, K), "vtav is NULL")
        refused(raw_semi(ctx, A, 0, D, K), "winv is NULL")
        refused(raw_semi(ctx, A, W, 0, K), "d is NULL")
        refused(raw_coef(ctx, A, 0, CF, K), "vtaav is NULL")
        refused(raw_coef(ctx, A, B, 0, K), "coef is NULL")
        refused(raw_rref(ctx, rows, 0, n, E, Z, I), "x is NULL")
        refused(raw_rref(ctx, rows, X, n, 0, Z, I), "e is NULL")
        refused(raw_rref(ctx, rows, X, n, E, Z, 0), "info is NULL")
        # one word short: 114 rows at a stride of 9 words are 1025 words; the allocation has 1024
        ld = 9
        assert ((rows - 1) * ld + n) * 8 == 8192 + 8
        short, sq, five, nw, n1 = (C.c_void_p() for _ in range(5))
        for hnd, size in ((short, 8192), (sq, n * n * 8 - 8), (five, 5 * n * n * 8 - 8), (nw, n * 8 - 8), (n1, (n + 1) * 8 - 8)):
            assert hip.hipMalloc(C.byref(hnd), C.c_size_t(size)) == 0
        try:
            refused(raw_semi(ctx, sq.value, W, D, K), " vtav ", "allocation ends")
            refused(raw_semi(ctx, A, sq.value, D, K), " winv ", "allocation ends")
            refused(raw_semi(ctx, A, W, nw.value, K), " d ", "allocation ends")
            refused(raw_coef(ctx, A, sq.value, CF, K), " vtaav ", "allocation ends")
            refused(raw_coef(ctx, A, B, five.value, K), " coef ", "allocation ends")
            refused(raw_rref(ctx, rows, short.value, ld, E, Z, I), " x ", "allocation ends")
            refused(raw_rref(ctx, rows, X, n, sq.value, Z, I), " e ", "allocation ends")
            refused(raw_rref(ctx, rows, X, n, E, sq.value, I), " z ", "allocation ends")
            refused(raw_rref(ctx, rows, X, n, E, Z, n1.value), " info ", "allocation ends")
            assert raw_rref(ctx, rows - 1, short.value, ld, ok[0].data_ptr(), 0, ok[1].data_ptr()) == blz.OK   # (one row fewer fits)
        finally:
            torch.cuda.synchronize()
            for hnd in (short, sq, five, nw, n1):
                assert hip.hipFree(hnd) == 0
        # ldx < n, rows < 0, a stride past 64-bit offsets
        refused(raw_rref(ctx, rows, X, n - 1, E, Z, I), " x ", "less than n")
        refused(raw_rref(ctx, rows, X, 0, E, Z, I), " x ", "less than n")
        refused(raw_rref(ctx, -1, X, n, E, Z, I), "rows = -1")
        refused(raw_rref(ctx, 1 << 40, X, 1 << 40, E, Z, I), "ldx", "beyond")
        with pytest.raises(ValueError):
            ctx.rref(x[:, :n - 1])
        # every forbidden overlap: an output with an input, an output with another output
        refused(raw_semi(ctx, Bp, Bp + 8, D, K), "winv overlaps vtav")
        refused(raw_semi(ctx, Bp, W, Bp + 8 * (n * n - 1), K), "d overlaps vtav")
        refused(raw_semi(ctx, Bp, W, D, Bp + 8 * (n * n - 1)), "npiv overlaps vtav")
        refused(raw_semi(ctx, A, Bp, Bp + 8 * (n * n - 1), K), "winv overlaps d")
        refused(raw_semi(ctx, A, Bp, D, Bp), "winv overlaps npiv")
        refused(raw_semi(ctx, A, W, Bp, Bp + 8 * (n - 1)), "d overlaps npiv")
        refused(raw_coef(ctx, Bp + 8 * (5 * n * n - 1), B, Bp, K), "coef overlaps vtav")
        refused(raw_coef(ctx, A, Bp, Bp + 8 * (n * n - 1), K), "coef overlaps vtaav")
        refused(raw_coef(ctx, Bp, B, CF, Bp), "npiv overlaps vtav")
        refused(raw_coef(ctx, A, Bp + 8, CF, Bp + 16), "npiv overlaps vtaav")
        refused(raw_coef(ctx, A, B, Bp, Bp + 8 * 3 * n * n), "coef overlaps npiv")
        refused(raw_rref(ctx, rows, Bp, n, Bp + 8 * n * (rows - 1), Z, I), "e overlaps x")
        refused(raw_rref(ctx, rows, Bp, n, E, Bp, I), "z overlaps x")
        refused(raw_rref(ctx, rows, Bp, n, E, Z, Bp + 8 * (rows * n - 1)), "info overlaps x")
        refused(raw_rref(ctx, rows, X, n, Bp, Bp + 8 * (n * n - 1), I), "e overlaps z")
        refused(raw_rref(ctx, rows, X, n, Bp + 8 * n, Z, Bp), "e overlaps info")
        refused(raw_rref(ctx, rows, X, n, E, Bp + 8 * n, Bp), "z overlaps info")
        # a capturing stream
        s = torch.cuda.Stream(device=DEV)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rcs, msgs = [], []
            for call in (lambda: raw_semi(ctx, A, W, D, K, h), lambda: raw_coef(ctx, A, B, CF, K, h),
                         lambda: raw_rref(ctx, rows, X, n, E, Z, I, h)):
                rcs.append(call())
                msgs.append(blz.lib().blz_last_error().decode())
            x.add_(0)                                   # (a graph of one node, not an empty one)
        assert rcs == [blz.EINVAL] * 3 and all("capturing" in m for m in msgs), (rcs, msgs)
        # nothing above ran: the outputs hold the sentinel, the inputs are what they were
        torch.cuda.synchronize()
        for t in (w, d, k, cf, e, z, info, both):
            assert (to_host(t) == np.uint64(SENTINEL)).all()
        assert np.array_equal(to_host(a), a0) and np.array_equal(to_host(b), b0) and np.array_equal(to_host(x), x0)
    # a context with the collectives forced on
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")           # read when the communicator is attached
    one = blz.LoopGroup(1)
    ctx = blz.Context(p, n)
    try:
        ctx.comm_init_loopback(one, 0)
        for call in (lambda: ctx.semi_inverse_device(a), lambda: ctx.ortho_coeffs(a, b, out=cf), lambda: ctx.rref(x)):
            with pytest.raises(blz.BlzError) as err:
                call()
            assert err.value.code == blz.EINVAL and "single rank" in str(err.value) and "BLZ_FORCE_COMM" in str(err.value)
    finally:
        ctx.close()
        one.close()
    torch.cuda.synchronize()
    assert (to_host(cf) == np.uint64(SENTINEL)).all()


def test_several_ranks_are_refused():
    p, n = P61, 4
    x = torch.zeros((100, n), dtype=torch.int64, device=DEV)
    a, cf, info = sentinel(n, n), sentinel(5, n, n), sentinel(n + 1)
    grp = blz.LoopGroup(2)
    ctxs = [blz.Context(p, n) for _ in range(2)]
    try:
        for r, c in enumerate(ctxs):
            c.comm_init_loopback(grp, r)
        for c in ctxs:
            refused(raw_semi(c, a.data_ptr(), cf.data_ptr(), info.data_ptr(), 0), "single rank")
            refused(raw_coef(c, a.data_ptr(), a.data_ptr(), cf.data_ptr(), 0), "single rank")
            refused(raw_rref(c, 100, x.data_ptr(), n, a.data_ptr(), 0, info.data_ptr()), "single rank")
    finally:
        for c in ctxs:
            c.close()
        grp.close()
    torch.cuda.synchronize()
    assert (to_host(cf) == np.uint64(SENTINEL)).all() and (to_host(info) == np.uint64(SENTINEL)).all()
