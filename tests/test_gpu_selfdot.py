"""The self-dot path of the iteration: v^T Av = tmp^T tmp out of the first product's kernel (k_spmv, self form),
v^T A^2 v = Av^T Av out of the second's (k_spmv_dot, self form), v not read again.

Inside the iteration tmp = B^T v and Av = B tmp for the same B (M or M^T), so v^T Av = v^T B B^T v = tmp^T tmp, and A = B B^T
is symmetric, so v^T A^2 v = (Av)^T (Av): both are products of a block with itself, exact sums mod p, the same words.

Case 1  past the chunk in the FIRST product: more than (chunk + 2) rows per lane group of k_spmv's grid (the plan of the
        first product), against fused_ref's closed form (test_gpu_fused_dot.check_iteration) -- and, in the signed and the wide
        value mode, against those modes' own closed forms.
Case 2  the new path against the old one (BLZ_NO_SELFDOT=1) on tiny systems, word for word, batches of 1, 2 and 5; one that
        stops inside a batch at both parities, one that passes through a step with some d[j] = 0.
Case 3  every condition that must switch the path off: selfdot_active == 0 and the oracle's words.
Case 4  get_block, set_block and a snapshot round trip between two batches.

Every case asserts Context.selfdot_active, so a case that does not reach its kernels fails.  (blz_get_small reads four of
the six n x n operands -- vtAv, vtAAv, winv, d; c and vtAvd have no getter and are compared through V and P, which the
update computes from them.)
"""
import os
import threading

import numpy as np
import pytest

import blz
import exact_ref as X
import fused_ref as F
import oracle as orc
import rhs_ref as R
import signed_ref as S
import wide_ref as Wd

import test_gpu_fused_dot as T
import test_gpu_signed as TS
import test_gpu_wide as TW

pytestmark = pytest.mark.gpu

P61, P57, P62 = T.P61, T.P57, T.P62
P31 = (1 << 31) - 1
PRIMES = T.PRIMES + (P31,)
SMALL = ((blz.VTAV, "vtAv"), (blz.VTAAV, "vtAAv"), (blz.WINV, "winv"), (blz.D, "d"))


def pid(p):
    return "p31w" if p == P31 else T.pid(p)


def stream_env(monkeypatch, xcd=None):
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_NO_STAGE", "1")
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    monkeypatch.delenv("BLZ_NO_SELFDOT", raising=False)
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    if xcd is not None:
        monkeypatch.setenv("BLZ_XCD_RANGES", str(xcd))


def first_groups(n):
    """Upper bound of the lane groups of the first product's launch: at most 8 workgroups per compute unit (and the round
    to whole XCD rounds), 256 / width groups each.  The case asserts the plan against it."""
    return ((T.cus() * 8 + 7) & ~7) * (256 // T.pow2(n))


def first_plan(ctx, right, p, n):
    """The plan of the first product on the self-dot path; returns its lane groups."""
    first = ctx.plan(not right)
    assert first["fused"] == 0 and first["plain"]["form"] == "spmv" and first["plain"]["split_log2"] == 0, first
    assert (first["n_medium"], first["n_heavy"], first["n_multi"]) == (0, 0, 0) and first["pieces"] == 1, first
    assert first["chunk"] == X.chunk(p) and first["width"] == T.pow2(n)
    return first["plain"]["grid_stream"] * 256 // first["width"], first


# ------------------------------------------------------------------------------------------------ case 1

CASES = []
for _k, _p in enumerate(PRIMES):
    CASES.append((_p, 8, True, _k % 2, _k))                  # tail batch on, XCD ranges off / on in turn
    CASES.append((_p, 8, False, (_k + 1) % 2, _k + 2))       # tail batch off, the other setting, the other orientation
# the other widths at a chunk of 1 and of 7 (rows grow with chunk x lane groups: 2^19 groups at n = 1), and at 32-bit words
# from a width of 4 on: the AccS accumulators have no chunk to pass, and 66 rows for each of 2^18 and more groups buy nothing
for _p in (P62, T.P60):
    CASES += [(_p, _n, None, _n % 2, _n + PRIMES.index(_p)) for _n in (1, 2, 4, 3, 5, 7)]
CASES += [(P31, _n, None, _n % 2, _n) for _n in (4, 3, 5, 7)]


@pytest.mark.parametrize("p,n,tail,xcd,k", CASES,
                         ids=[f"{pid(p)}-n{n}-tail{'x' if t is None else int(t)}-xcd{x}-{k % 4}" for p, n, t, x, k in CASES])
def test_first_product_past_chunk_rows_per_lane_group(monkeypatch, p, n, tail, xcd, k):
    """A scattered permutation plus a ladder of rows of 0 ... 64 entries; k picks the orientation, the operand and the way the
    values are stored."""
    stream_env(monkeypatch, xcd)
    rows = T.rows_past_chunk(p, first_groups(n))
    if tail is False:
        rows = max(rows, T.TAIL_NNZ + 1)
    elif tail is True and rows >= T.TAIL_NNZ - 1000:
        tail = None     # (chunk 64: the rows past the chunk are already more entries than a slab with the tail batch has)
    right, kind = T.variant(k)
    A = F.mixed([F.perm(rows, seed=k + 1, mode=("ones", "palette", "array")[k % 3]), F.ladder(T.SHORT, repeat=3, mode="palette")])
    with blz.Context(p, n) as ctx:
        assert ctx.word_bytes == (4 if p == P31 else 8)
        ctx.set_matrix(T.to_blz(A, right, p), right)
        pl = T.fused_plan(ctx, right, "spmv", n)
        groups, first = first_plan(ctx, right, p, n)
        assert ctx.selfdot_active == 1
        # the first product's output (tmp: one row per column of A) past the chunk in every lane group of its launch
        assert A.ncols >= T.rows_past_chunk(p, groups), (A.ncols, first)
        assert A.nrows >= T.rows_past_chunk(p, T.stream_accumulators(pl)), (A.nrows, pl)
        assert first["tail_batch"] == pl["tail_batch"] == (A.nnz < T.TAIL_NNZ)
        if tail is not None:
            assert first["tail_batch"] == int(tail)
        assert first["plain"]["xcd_ranges"] == xcd and pl["dot"]["xcd_ranges"] == xcd, (first, pl)
        T.check_iteration(ctx, A, p, n, right, (kind,))
        assert ctx.selfdot_active == 1


MODE_CASES = [("signed", P62, "palette", "ramp"), ("signed", P61, "array", "max"), ("signed", T.P60, "array", "ramp"),
              ("wide", P62, "palette", "max"), ("wide", P61, "array", "ramp"), ("wide", T.P61B, "allmax", "max")]


@pytest.mark.parametrize("vm,p,mode,kind", MODE_CASES, ids=[f"{v}-{T.pid(p)}-{m}-{k}" for v, p, m, k in MODE_CASES])
def test_first_product_past_chunk_signed_and_wide_values(monkeypatch, vm, p, mode, kind):
    """The other two value modes (64-bit words, a left kernel: what their closed forms cover), past the chunk of the first
    product in every lane group."""
    n = 8
    stream_env(monkeypatch, 0)
    rows = T.rows_past_chunk(p, first_groups(n))
    shape = F.mixed([F.perm(rows, seed=11), F.ladder(T.SHORT, repeat=3)])
    if vm == "signed":
        A = S.with_signed_values(shape, mode, seed=3)
        ctx = TS.signed_context(p, n, TS.to_blz(A))
    else:
        A = Wd.with_wide_values(shape, mode, p, seed=3)
        ctx = TW.wide_context(p, n, TW.to_blz(A))
    with ctx:
        assert (ctx.slab_signed(False) and ctx.slab_signed(True)) if vm == "signed" else (ctx.slab_wide(False) and ctx.slab_wide(True))
        groups, first = first_plan(ctx, False, p, n)
        assert ctx.plan(False)["fused"] == 1 and ctx.selfdot_active == 1
        assert A.ncols >= T.rows_past_chunk(p, groups), (A.ncols, first)
        (TS if vm == "signed" else TW).check_iteration(ctx, A, n, p, (kind,))
        assert ctx.selfdot_active == 1


# ------------------------------------------------------------------------------------------------ case 2


@pytest.fixture
def tiny_env(monkeypatch):
    """The tiny systems in the numbering of the file and in the streaming form (a renumbering would plan an LDS panel)."""
    for key in ("BLZ_NO_REORDER", "BLZ_NO_STAGE", "BLZ_NO_PANEL"):
        monkeypatch.setenv(key, "1")
    for key in ("BLZ_GRAPH", "BLZ_NO_SELFDOT", "BLZ_NO_FUSE", "BLZ_STAGE_ALWAYS", "BLZ_FORCE_COMM", "BLZ_EXPLICIT_P"):
        monkeypatch.delenv(key, raising=False)


def as_orc(M):
    return orc.Matrix(M.nrows, M.ncols, M.i, M.j, M.x)


def tiny(seed=0x53454C46):
    """A few hundred rows, fewer than eight entries a row on either side: whole rows per lane group in both products."""
    return blz.Matrix.synth(300, 260, 1500, seed, P61)


def state(ctx):
    """Everything a caller can see, V and the operands before P (reading P makes it explicit)."""
    out = {"iterations": ctx.iterations, "implicit": ctx.p_implicit}
    for which, name in SMALL:
        out[name] = ctx.get_small(which)
    out["v"], out["tmp"], out["av"] = ctx.get_block(blz.V), ctx.get_block(blz.TMP), ctx.get_block(blz.AV)
    out["p"] = ctx.get_block(blz.P)
    return out


def same_state(a, b, where):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), (where, key)


def two_paths(monkeypatch, M, n, right, script):
    """script(ctx) -> list of states; run on the self-dot path and under BLZ_NO_SELFDOT=1, compared word for word."""
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("BLZ_NO_SELFDOT", "1")
        else:
            monkeypatch.delenv("BLZ_NO_SELFDOT", raising=False)
        with blz.Context(P61, n) as ctx:
            ctx.set_matrix(M, right)
            assert ctx.plan(right)["fused"] == 1
            assert ctx.selfdot_active == (0 if off else 1), ctx.plan(not right)
            ctx.init_v()
            runs.append(script(ctx))
            assert ctx.selfdot_active == (0 if off else 1)
    assert len(runs[0]) == len(runs[1]) > 0
    for q, (a, b) in enumerate(zip(*runs)):
        same_state(a, b, q)
    return runs[0]


@pytest.mark.parametrize("mfma", [True, False], ids=["rotating", "explicit"])
@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("n", [8, 4, 5])
def test_new_path_against_old_path(monkeypatch, tiny_env, n, right, mfma):
    """iterate(k) for k = 1, 2, 5 on both paths, with the matrix-core update (p implicit, the buffers change places) and
    without; the last state also against the oracle."""
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    if mfma:
        monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    M = tiny()

    def script(ctx):
        out = []
        for k in (1, 2, 5):
            done, stopped, _ = ctx.iterate(k)
            out.append(dict(state(ctx), done=done, stopped=stopped))
        return out

    last = two_paths(monkeypatch, M, n, right, script)[-1]
    want = orc.block_lanczos(as_orc(M), n, P61, right=right, stop_after=8)
    assert last["iterations"] == want["iterations"] == 8 and not last["stopped"]
    assert np.array_equal(last["v"], want["v"]) and np.array_equal(last["p"], want["p"])


def test_stop_inside_a_batch_at_both_parities(monkeypatch, tiny_env):
    """The solve ends inside the batch; the steps enqueued past the stop are no-ops on both paths, and the host's swaps are
    reconciled the same way: an even and an odd number of them."""
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    n, M = 8, tiny(0x53544F50)
    want = orc.block_lanczos(as_orc(M), n, P61)
    steps = want["iterations"]
    assert 2 < steps < 200
    seen = set()
    for extra in (7, 8):
        def script(ctx, extra=extra):
            done, stopped, _ = ctx.iterate(steps + extra)
            first = dict(state(ctx), done=done, stopped=stopped)
            again = ctx.iterate(3)
            return [first, dict(state(ctx), done=again[0], stopped=again[1])]

        a, b = two_paths(monkeypatch, M, n, False, script)
        assert a["done"] == steps and a["stopped"] and b["done"] == 0 and b["stopped"]
        assert np.array_equal(a["v"], want["v"]) and np.array_equal(a["p"], want["p"])
        assert np.array_equal(b["v"], want["v"]) and np.array_equal(b["p"], want["p"])
        seen.add(extra % 2)
    assert seen == {0, 1}


def test_a_step_with_a_zero_in_d(monkeypatch, tiny_env):
    """fast, fast | a column of v copied over another (the next step has d[j] = 0 and meets the carried E) | on, unseen."""
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    n, M = 8, tiny()
    Mo = as_orc(M)
    recs = []
    end = orc.block_lanczos(Mo, n, P61, stop_after=2, trace=recs.append)
    v2 = end["v"].reshape(-1, n).copy()
    v2[:, 3] = v2[:, 5]
    v2 = v2.reshape(-1)
    recs_b = []
    end_b = orc.block_lanczos(Mo, n, P61, stop_after=5, trace=recs_b.append, v_init=v2, p_init=end["p"], start_iter=2)
    assert end_b["iterations"] == 5 and not recs_b[0]["d"].all() and recs_b[0]["npiv"] > 0

    def script(ctx):
        ctx.iterate(2)
        ctx.set_block(blz.V, v2)
        assert ctx.p_implicit == 1
        done, stopped, _ = ctx.iterate(1)
        d1 = ctx.get_small(blz.D)
        more = ctx.iterate(2)
        return [dict(state(ctx), d1=d1, done=done + more[0], stopped=stopped or more[1])]

    got = two_paths(monkeypatch, M, n, False, script)[0]
    assert np.array_equal(got["d1"], recs_b[0]["d"]) and not got["d1"].all()
    assert got["iterations"] == 5 and np.array_equal(got["v"], end_b["v"]) and np.array_equal(got["p"], end_b["p"])


# ------------------------------------------------------------------------------------------------ case 3


def against_oracle(ctx, M, n, right, steps=3):
    ctx.init_v()
    assert ctx.iterate(steps)[:2] == (steps, False)
    want = orc.block_lanczos(as_orc(M), n, P61, right=right, stop_after=steps)
    assert np.array_equal(ctx.get_block(blz.V), want["v"]) and np.array_equal(ctx.get_block(blz.P), want["p"])


FALLBACK_ENV = {"stage_always": {"BLZ_STAGE_ALWAYS": "1"}, "no_fuse": {"BLZ_NO_FUSE": "1"}, "graph": {"BLZ_GRAPH": "1"},
                "no_selfdot": {"BLZ_NO_SELFDOT": "1"}}


@pytest.mark.parametrize("name", sorted(FALLBACK_ENV))
def test_fallback_by_switch(monkeypatch, tiny_env, name):
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    n, M = 8, tiny()
    with blz.Context(P61, n) as ctx:            # the same matrix takes the path without the switch
        ctx.set_matrix(M, False)
        assert ctx.selfdot_active == 1
    for key, val in FALLBACK_ENV[name].items():
        monkeypatch.setenv(key, val)
    if name == "stage_always":
        monkeypatch.delenv("BLZ_NO_STAGE")
    with blz.Context(P61, n) as ctx:
        assert ctx.selfdot_active == 0          # no matrix yet
        ctx.set_matrix(M, False)
        assert ctx.selfdot_active == 0
        against_oracle(ctx, M, n, False)
        assert ctx.selfdot_active == 0


def test_fallback_forced_collectives(monkeypatch, tiny_env):
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")
    n, M = 8, tiny()
    with blz.Context(P61, n) as ctx:
        ctx.comm_init(blz.comm_unique_id(), 0, 1)
        ctx.set_matrix(M, False, 0, 1)
        assert ctx.selfdot_active == 0
        against_oracle(ctx, M, n, False)


def test_fallback_width_16(tiny_env):
    n, M = 16, tiny()
    with blz.Context(P61, n) as ctx:
        ctx.set_matrix(M, False)
        assert ctx.plan(False)["fused"] == 0 and ctx.selfdot_active == 0
        against_oracle(ctx, M, n, False)


@pytest.mark.parametrize("length", [65, 3000], ids=["medium", "heavy"])
@pytest.mark.parametrize("side", ["first", "second"])
def test_fallback_outlier_row(monkeypatch, length, side):
    """One row above the outlier threshold in the slab of the first or of the second product: the whole step goes the old
    way (closed form, as in test_gpu_fused_dot)."""
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_NO_STAGE", "1")
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    n, p = 8, P57
    base = F.mixed([F.perm(T.pad_rows(n), seed=3), F.ladder((length,), repeat=1, mode="palette")])
    for right in (False, True):
        # A's rows are the second product's output rows; its transpose carries the long row into the first product's slab
        A = base if side == "second" else F.Coo(base.ncols, base.nrows, base.j, base.i, base.x)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(T.to_blz(A, right, p), right)
            second, first = ctx.plan(right), ctx.plan(not right)
            long_one = second if side == "second" else first
            assert long_one["n_medium"] + long_one["n_heavy"] >= 1 and second["fused"] == 1, (first, second)
            assert ctx.selfdot_active == 0
            T.check_iteration(ctx, A, p, n, right, ("ramp",))


def test_fallback_border(monkeypatch):
    """A right-hand side set: the bordered operator's step goes the old way (exact_ref's trajectory of the augmented matrix)."""
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    n, p = 8, P61
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rand300x200.mtx")
    Mb, Mx = blz.Matrix.load(path, p), X.load_mtx(path, p)
    for right in (False, True):
        x0, b = R.planted(Mx, right, p, 11)
        recs, end = X.trajectory(R.augmented(Mx, b, right), n, p, right)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix_rhs(Mb, R.as_u64(b), right)
            assert ctx.has_rhs and ctx.selfdot_active == 0
            ctx.init_v()
            for it, rec in enumerate(recs[:4]):
                assert [int(w) for w in ctx.get_block(blz.V)] == rec["v"], (it, "v")
                ctx.iterate(1)
                for which, key in SMALL:
                    assert [int(w) for w in ctx.get_small(which)] == [int(w) for w in rec[key]], (it, key)
            assert ctx.selfdot_active == 0


def test_fallback_two_loopback_ranks(tiny_env):
    n, M = 8, tiny()
    want = orc.block_lanczos(as_orc(M), n, P61, stop_after=3)
    group = blz.LoopGroup(2)
    out, errs = [None, None], [None, None]

    def rank_main(g):
        try:
            with blz.Context(P61, n) as ctx:
                ctx.comm_init_loopback(group, g)
                ctx.set_matrix(M, False, g, 2)
                active = ctx.selfdot_active
                ctx.init_v()
                assert ctx.iterate(3)[:2] == (3, False)
                out[g] = (active, ctx.get_block(blz.V), ctx.get_block(blz.P))
        except BaseException as e:          # noqa: BLE001 (re-raised below)
            errs[g] = e

    ths = [threading.Thread(target=rank_main, args=(g,)) for g in range(2)]
    try:
        for t in ths:
            t.start()
        for t in ths:
            t.join(600)
    finally:
        group.close()
    for e in errs:
        if e is not None:
            raise e
    assert [q[0] for q in out] == [0, 0]
    assert np.array_equal(out[0][1] | out[1][1], want["v"]) and np.array_equal(out[0][2] | out[1][2], want["p"])


# ------------------------------------------------------------------------------------------------ case 4


def test_consumers_between_batches(monkeypatch, tiny_env):
    """get_block, set_block and a snapshot round trip between two batches on the self-dot path, against the oracle."""
    monkeypatch.delenv("BLZ_GRAPH", raising=False)
    monkeypatch.delenv("BLZ_NO_SELFDOT", raising=False)
    monkeypatch.setenv("BLZ_MFMA_MIN_ROWS", "0")
    n, M = 8, tiny()
    Mo = as_orc(M)
    recs = []
    end = orc.block_lanczos(Mo, n, P61, stop_after=7, trace=recs.append)
    with blz.Context(P61, n) as ctx:
        ctx.set_matrix(M, False)
        assert ctx.selfdot_active == 1
        ctx.init_v()
        assert ctx.iterate(3)[:2] == (3, False)
        assert np.array_equal(ctx.get_small(blz.VTAV), recs[2]["vtAv"]) and np.array_equal(ctx.get_small(blz.VTAAV), recs[2]["vtAAv"])
        assert np.array_equal(ctx.get_block(blz.V), recs[3]["v"])
        ctx.snapshot_begin()
        sv, sp, its = ctx.snapshot_wait()
        assert its == 3 and np.array_equal(sv, recs[3]["v"]) and np.array_equal(sp, recs[3]["p"])
        assert ctx.iterate(2)[:2] == (2, False)
        assert np.array_equal(ctx.get_block(blz.V), recs[5]["v"]) and np.array_equal(ctx.get_block(blz.P), recs[5]["p"])
        assert np.array_equal(ctx.get_block(blz.TMP), ctx.get_block(blz.TMP))
        # a caller's own blocks from here: the oracle continues from the same (v, p)
        q = np.random.default_rng(7).integers(0, P61, size=M.nrows * n, dtype=np.uint64)
        ctx.set_block(blz.V, q)
        ctx.set_block(blz.P, recs[5]["p"])
        want = orc.block_lanczos(Mo, n, P61, stop_after=7, v_init=q, p_init=recs[5]["p"], start_iter=5)
        assert ctx.selfdot_active == 1 and ctx.iterate(2)[:2] == (2, False)
        assert np.array_equal(ctx.get_block(blz.V), want["v"]) and np.array_equal(ctx.get_block(blz.P), want["p"])
    assert end["iterations"] == 7
