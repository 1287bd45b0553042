"""M X = B and X M = B on several ranks: the dense border distributed over the row partition, against exact integers.

Every rank keeps its own rows of tmp and of B.  The border update reads the k border rows of its operand from the gathered
copy; the border dot is taken over the rank's rows, its k x n words are all-reduced and the owners of the border rows store
them (csrc/blz_border.hip: k_border_finalize_send, k_border_place; k_border_rows_send for the solution).  The ranks here
are loopback ranks, threads of one process on one GPU as in tests/test_gpu_loopback.py, and the truth is the augmented
matrix in Python integers (rhs_block_ref / rhs_ref / exact_ref):

A. the two products alone, through blz_spmv, at every reducer class, 2 / 3 / 8 ranks, k = 1, 3, 16;
B. border rows on more than one rank: the whole trajectory and a batch past the stop;
C. whole solves against the one-rank context and the planted solutions;
D. one rank with the RCCL collectives forced on, and two real devices where there are two;
E. what is refused, collectively, and what is planned;
F. the command line's --rhs-gpus.
"""
import ctypes as C
import functools
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import blz
import exact_ref as X
import rhs_block_ref as RB
import rhs_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIBDIR = os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "lib")
EXE, CHECKER = os.path.join(LIBDIR, "lanczos_modp"), os.path.join(LIBDIR, "checker_modp")
P61 = X.P61
NDEV = blz.device_count()


def mpath(name):
    return os.path.join(GOLDEN, name + ".mtx")


@functools.lru_cache(maxsize=None)
def pair(name, p):
    return blz.Matrix.load(mpath(name), p), X.load_mtx(mpath(name), p)


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


def together(parts):
    full = np.zeros_like(parts[0])
    for q in parts:                      # a rank returns its own rows, zeros elsewhere
        full |= q
    return full


def ints(a):
    return [int(w) for w in a]


# ------------------------------------------------------------------------------------------------- A. the two products alone

# 32-bit words (Barrett low and at the top of u32, the reference's cap, and the folding 2^31-1, whose all-reduced sums
# k_border_place reduces by Barrett like the others), 64-bit words: the folding 2^61-1, a Barrett prime just below 2^61
# (8 p <= 2^64 still holds) and one just below 2^62, where 3 ranks are the most that nranks * p <= 2^64 allows
A_PRIMES = (65537, 4294967291, (1 << 30) - 35, X.P31, P61, 2305843009213693907, 4611686018427387847)
A_CASES = [(p, nranks) for p in A_PRIMES for nranks in (2, 3, 8) if nranks * p <= 1 << 64]
PADDED = {1: (1,), 3: (3,), 8: (1, 3), 16: (1, 3, 16), 64: (1, 3, 16)}      # width -> the k for which it is one of k, 8, 16, 64
EXACT = {1: (1,), 3: (1, 3), 5: (1, 3)}                                      # BLZ_NO_PAD=1: widths 1, 3, 5


def operands(kind, M, right, n, p, k, seed):
    """(the k right-hand sides, block of side 0 with the k border rows last, block of side 1) of one kind"""
    rnd = np.random.default_rng(seed)
    n0, n1 = (M.ncols if right else M.nrows) + k, (M.nrows if right else M.ncols)

    def words(count):
        if kind == "max":
            return [p - 1] * count
        return [int(w) % p for w in rnd.integers(0, 1 << 62, size=count, dtype=np.uint64)]

    return [words(n1) for _ in range(k)], words(n0 * n), words(n1 * n)


def products_on_ranks(Mb, Mx, right, n, p, ks, nranks):
    """every (k, kind): the product that writes side 1 and the one that writes side 0 (into AV and into P), on nranks
    loopback ranks, each rank's rows put together and compared with the restatement word for word"""
    ops = {(k, kind): operands(kind, Mx, right, n, p, k, 1000 * n + 10 * k + s) for k in ks for s, kind in enumerate(("random", "max"))}
    got = [dict() for _ in range(nranks)]
    group = blz.LoopGroup(nranks)

    def rank_main(g):
        with blz.Context(p, n) as ctx:
            ctx.comm_init_loopback(group, g)
            for k in ks:
                for s, kind in enumerate(("random", "max")):
                    cols, v, t = ops[(k, kind)]
                    if s == 0:          # the one-call form, then a second border on the same matrix
                        ctx.set_matrix_rhs_ranks(Mb, RB.rows(cols), right, g, nranks)
                    else:
                        ctx.set_rhs_ranks(RB.rows(cols))
                    assert ctx.has_rhs and ctx.rhs_count == k and ctx.rows(blz.V) == (Mx.ncols if right else Mx.nrows) + k
                    ctx.set_block(blz.V, R.as_u64(v))
                    ctx.spmv(not right, blz.V, blz.TMP)
                    upd = ctx.get_block(blz.TMP)
                    ctx.set_block(blz.TMP, R.as_u64(t))
                    dots = []
                    for dst in (blz.AV, blz.P):
                        ctx.spmv(right, blz.TMP, dst)
                        dots.append(ctx.get_block(dst))
                    got[g][(k, kind)] = (upd, dots[0], dots[1])

    try:
        run_ranks(nranks, rank_main)
    finally:
        group.close()
    for (k, kind), (cols, v, t) in ops.items():
        A = RB.augmented(Mx, cols, right)
        want = X.spmv(A, v, not right, n, p)
        have = ints(together([q[(k, kind)][0] for q in got]))
        assert have == want, (k, n, kind, "update", next(q for q in range(len(want)) if have[q] != want[q]))
        want = X.spmv(A, t, right, n, p)
        for which in (1, 2):
            have = ints(together([q[(k, kind)][which] for q in got]))
            assert have == want, (k, n, kind, "dot", which, next(q for q in range(len(want)) if have[q] != want[q]))


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p,nranks", A_CASES)
def test_border_products_alone_on_loopback_ranks(monkeypatch, p, nranks, right):
    """quirks40x30 with k = 1, 3, 16 at the widths k, 8, 16, 64 (padded) and 1, 3, 5 (BLZ_NO_PAD=1), random operands and all
    p - 1 with all p - 1 right-hand sides: at 8 ranks and 2^61 - 1 the largest sum the all-reduce may carry; the 32-bit primes
    take the 4-byte store of k_border_place.  Some of the 8 ranks hold no row of tmp at all and send zeros."""
    Mb, Mx = pair("quirks40x30", p)
    for n, ks in PADDED.items():
        products_on_ranks(Mb, Mx, right, n, p, ks, nranks)
    monkeypatch.setenv("BLZ_NO_PAD", "1")
    for n, ks in EXACT.items():
        products_on_ranks(Mb, Mx, right, n, p, ks, nranks)


# ------------------------------------------------------------------------------------------------- whole solves on ranks


def solve_on_ranks(Mb, cols, p, n, right, nranks, batch=16, extra=0, attach=None, devices=False):
    """every rank: context, communicator, its slabs and its rows of the k right-hand sides, blz_iterate to the stop (and `extra`
    iterations beyond), the solution call; returns what each rank holds"""
    k = len(cols)
    B = RB.rows(cols)
    group = blz.LoopGroup(nranks) if attach is None else None
    out = [None] * nranks

    def rank_main(g):
        with blz.Context(p, n, g if devices else 0) as ctx:
            if attach is None:
                ctx.comm_init_loopback(group, g)
            else:
                attach(ctx, g)
            ctx.set_matrix_rhs_ranks(Mb, B, right, g, nranks)
            assert ctx.has_rhs and ctx.rhs_count == k
            rows0 = ctx.rows(blz.V)
            pieces = (ctx.exchange_pieces(False), ctx.exchange_pieces(True))
            fused = [ctx.plan(t, pieces[t] - 1)["fused"] for t in (False, True)]
            ctx.init_v()
            while not ctx.iterate(batch)[1]:
                pass
            if extra:
                assert ctx.iterate(extra)[:2] == (0, True)           # a whole batch past the stop
            rec = dict(its=ctx.iterations, v=ctx.get_block(blz.V), p=ctx.get_block(blz.P), tmp=ctx.get_block(blz.TMP),
                       small=[ctx.get_small(q) for q in (blz.VTAV, blz.VTAAV, blz.WINV)], check=ctx.final_check(),
                       owners=[ctx.owner_of_row(blz.V, rows0 - k + i) for i in range(k)], pieces=pieces, fused=fused,
                       short=(ctx.short_side(False), ctx.short_side(True)), local=ctx.local_rows(blz.V)[1])
            if k == 1:
                status, x = ctx.solution()
                rec.update(status=[status], x=None if x is None else x.reshape(-1, 1))
            else:
                rec["status"], rec["x"] = ctx.solution_block()
            rec.update(v_end=ctx.get_block(blz.V), tmp_end=ctx.get_block(blz.TMP))
            out[g] = rec

    try:
        run_ranks(nranks, rank_main)
    finally:
        if group:
            group.close()
    return out


def merged_x(got, rows, k):
    """the ranks' rows of x put together (None where no system was solved and the call left x alone)"""
    if all(q["x"] is None for q in got):
        return None
    return together([q["x"] if q["x"] is not None else np.zeros((rows, k), dtype=np.uint64) for q in got])


@functools.lru_cache(maxsize=None)
def one_rank(name, p, n, right, case):
    """(statuses, x, iterations) of the plain one-rank context for the right-hand sides of `case`: computed once"""
    Mb, Mx = pair(name, p)
    cols = rhs_of(Mx, right, p, case)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix_rhs_block(Mb, RB.rows(cols), right)
        ctx.init_v()
        while not ctx.iterate(16)[1]:
            pass
        status, x = ctx.solution_block()
        return status, x, ctx.iterations


def rhs_of(Mx, right, p, case):
    kind, k, seed = case
    if kind == "planted":
        return RB.planted(Mx, right, p, k, seed)[1]
    if kind == "mixed":          # the planted block with column 1 replaced by a random b
        cols = RB.planted(Mx, right, p, k, seed)[1]
        cols[1] = R.random_rhs(Mx, right, p, seed)
        return cols
    return [R.random_rhs(Mx, right, p, seed + i) for i in range(k)]       # "random": inconsistent systems


@functools.lru_cache(maxsize=None)
def verdict(name, p, n, right, case):
    Mx = pair(name, p)[1]
    return RB.verdict(Mx, rhs_of(Mx, right, p, case), right, n, p)


# ------------------------------------------------------------------------------------------------- B. border rows on two ranks


@pytest.mark.parametrize("reorder", (False, True))
@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (P61, 65537))
def test_border_rows_on_more_than_one_rank(monkeypatch, p, right, reorder):
    """synth(40, 30, 40), k = n = 16 on 8 ranks: the 16 empty border rows fall on the last two ranks of the nnz-balanced partition
    (file numbering: 4 + 12 rows for x M = B, 5 + 11 for M x = B).  The whole solve and 20 iterations past the stop against
    exact_ref.trajectory of the augmented matrix."""
    if not reorder:
        monkeypatch.setenv("BLZ_NO_REORDER", "1")
    n = k = 16
    nranks = 8
    Mb = blz.Matrix.synth(40, 30, 40, 0x4C4F4F50, p)
    Mx = X.Coo(Mb.nrows, Mb.ncols, ints(Mb.i), ints(Mb.j), ints(Mb.x))
    cols = RB.planted(Mx, right, p, k, 71)[1]
    got = solve_on_ranks(Mb, cols, p, n, right, nranks, batch=7, extra=20)
    owners = got[0]["owners"]
    assert all(q["owners"] == owners for q in got)
    if not reorder:
        assert [owners.count(g) for g in (6, 7)] == ([5, 11] if right else [4, 12]), owners
    assert len(set(owners)) >= 2, owners            # before anything is compared: the case is the one this test is about
    _, end = X.trajectory(RB.augmented(Mx, cols, right), n, p, right)
    assert all(q["its"] == end["iterations"] for q in got)
    for key in ("v", "p", "tmp"):
        assert ints(together([q[key] for q in got])) == end[key], key
    for q in got:
        assert all((s < p).all() for s in q["small"])
        assert all(np.array_equal(a, b) for a, b in zip(q["small"], got[0]["small"]))
        assert q["check"] == (any(end["v"]), not any(end["tmp"]))
        assert q["fused"] == [0, 0]
    want = RB.verdict(Mx, cols, right, n, p)["solvable"]
    for q in got:
        assert q["status"] == got[0]["status"]
    assert [int(s == 0) for s in got[0]["status"]] == want and set(got[0]["status"]) <= {0, 1}
    x = merged_x(got, (Mx.ncols if right else Mx.nrows), k)
    for i, (xi, b) in enumerate(zip(RB.columns(x), cols)):
        if got[0]["status"][i] == 0:
            assert not any(R.residual(Mx, xi, b, right, p)), i
        else:
            assert not any(xi), i


# ------------------------------------------------------------------------------------------------- C. whole solves

SOLVES = (("rand300x200", True, 65537, 8, ("planted", 3, 51), [1, 1, 1], True),
          ("wide120x260", False, P61, 8, ("planted", 3, 51), [1, 1, 1], True),
          ("rand300x200", True, 65537, 8, ("mixed", 3, 53), [1, 0, 1], True),
          ("rand300x200", True, 65537, 4, ("planted", 1, 41), [1], True),
          ("rand300x200", True, 65537, 8, ("random", 2, 54), [0, 0], False))


@pytest.mark.parametrize("chunks", (None, "3"))
@pytest.mark.parametrize("nranks", (2, 3, 8))
@pytest.mark.parametrize("name,right,p,n,case,solvable,unique", SOLVES)
def test_whole_solves_on_loopback_ranks(monkeypatch, name, right, p, n, case, solvable, unique, nranks, chunks):
    """Statuses identical on every rank; x put together from the ranks' rows equal to the one-rank context's word for word,
    equal to the planted x where that is the only solution, residual zero in Python integers."""
    Mb, Mx = pair(name, p)
    cols = rhs_of(Mx, right, p, case)
    k = len(cols)
    ref = verdict(name, p, n, right, case)
    assert ref["solvable"] == solvable                                  # on the CPU first: a miss below is the GPU's
    if case[0] == "random":
        assert all(R.solve(Mx, b, right, p)[1] is None for b in cols)
    one_status, one_x, one_its = one_rank(name, p, n, right, case)
    assert [int(s == 0) for s in one_status] == solvable and one_its == ref["iterations"]
    if chunks:
        monkeypatch.setenv("BLZ_AG_CHUNKS", chunks)
    got = solve_on_ranks(Mb, cols, p, n, right, nranks, batch=13)
    if chunks:
        assert got[0]["pieces"] == (int(chunks), int(chunks))
    rows = Mx.ncols if right else Mx.nrows
    for q in got:
        assert q["status"] == one_status and q["its"] == ref["iterations"] and q["fused"] == [0, 0]
        assert q["short"] == (False, False)
    assert X.sha(together([q["v"] for q in got])) == ref["v_sha"]
    x = merged_x(got, rows, k)
    if not any(solvable):
        # nothing solved: blz_solution_block leaves zero columns, blz_solution leaves x alone
        assert x is None or not x.any()
        return
    assert x.shape == one_x.shape and np.array_equal(x, one_x)
    # a rank writes the rows it owns and no others
    assert sum(q["local"] for q in got) == rows + k
    x0s = RB.planted(Mx, right, p, k, case[2])[0]
    for i, (xi, b) in enumerate(zip(RB.columns(x), cols)):
        if solvable[i]:
            assert not any(R.residual(Mx, xi, b, right, p)), i
            if unique:
                assert xi == x0s[i], i
        else:
            assert not any(xi), i
    # V keeps (y_i, -e_i) in column i where system i is solved, TMP the zero product, on every rank's rows
    V = together([q["v_end"] for q in got]).reshape(-1, n)
    for i in range(k):
        if solvable[i]:
            assert np.array_equal(V[:-k, i], x[:, i]) and ints(V[-k:, i]) == [(p - 1) if q == i else 0 for q in range(k)]
        else:
            assert not V[:, i].any()
    assert not V[:, k:].any() and not together([q["tmp_end"] for q in got]).any()


def test_the_recorded_large_case_on_three_ranks():
    """rand3000x2000, n = 16, k = 5, p = 2^61 - 1 (rhs_block_ref.recorded): the ranks stop on the block of the recorded hash and
    solve what the restatement's final block solves."""
    c = RB.RECORDED_CASE
    p, n, k, right = c["p"], c["n"], c["k"], c["right"]
    ref = RB.recorded()
    assert ref["w_rank"] == k and all(ref["solvable"])
    Mb, Mx = pair(c["name"], p)
    cols = RB.planted(Mx, right, p, k, c["seed"])[1]
    got = solve_on_ranks(Mb, cols, p, n, right, 3, batch=32)
    assert all(q["status"] == [0] * k and q["its"] == ref["iterations"] for q in got)
    assert X.sha(together([q["v"] for q in got])) == ref["v_sha"]
    x = merged_x(got, Mx.ncols, k)
    for xi, b in zip(RB.columns(x), cols):
        assert not any(R.residual(Mx, xi, b, right, p))


# ------------------------------------------------------------------------------------------------- D. RCCL


@pytest.mark.parametrize("forced", (True, False))
def test_one_rank_with_the_rccl_exchange_forced_on(monkeypatch, forced):
    """BLZ_FORCE_COMM=1 on a one-rank RCCL communicator: the real ncclAllReduce carries the border words (and the real
    ncclAllGather the operand, in three pieces).  Without the switch a one-rank communicator exchanges nothing and the new
    entry points still take the context (the old ones refuse any communicator)."""
    if forced:
        monkeypatch.setenv("BLZ_FORCE_COMM", "1")
        monkeypatch.setenv("BLZ_AG_CHUNKS", "3")
    name, right, p, n, case = "rand300x200", True, 65537, 8, ("planted", 3, 51)
    Mb, Mx = pair(name, p)
    cols = rhs_of(Mx, right, p, case)
    assert verdict(name, p, n, right, case)["solvable"] == [1, 1, 1]
    uid = blz.comm_unique_id()
    got = solve_on_ranks(Mb, cols, p, n, right, 1, attach=lambda ctx, g: ctx.comm_init(uid, 0, 1))
    assert got[0]["status"] == [0, 0, 0] and got[0]["pieces"] == ((3, 3) if forced else (1, 1)) and got[0]["fused"] == [0, 0]
    assert RB.columns(got[0]["x"]) == RB.planted(Mx, right, p, 3, 51)[0]
    if forced:
        monkeypatch.delenv("BLZ_FORCE_COMM")
        monkeypatch.delenv("BLZ_AG_CHUNKS")
    assert np.array_equal(got[0]["x"], one_rank(name, p, n, right, case)[1])


@pytest.mark.skipif(NDEV < 2, reason=f"needs >= 2 GPUs ({NDEV} visible)")
def test_two_devices_with_a_real_communicator():
    name, right, p, n, case = "rand300x200", True, 65537, 8, ("planted", 3, 51)
    Mb, Mx = pair(name, p)
    cols = rhs_of(Mx, right, p, case)
    uid = blz.comm_unique_id()
    got = solve_on_ranks(Mb, cols, p, n, right, 2, attach=lambda ctx, g: ctx.comm_init(uid, g, 2), devices=True)
    assert all(q["status"] == [0, 0, 0] for q in got)
    assert RB.columns(merged_x(got, Mx.ncols, 3)) == RB.planted(Mx, right, p, 3, 51)[0]


# ------------------------------------------------------------------------------------------------- E. refusals and plans


def refused_on_every_rank(nranks, p, n, prepare, call, fragments):
    """every rank runs prepare(ctx, g), then call(ctx, g) must fail with BLZ_EINVAL on every rank (no rank is left waiting);
    fragments: what at least one rank's message must hold, the others may say that another rank refused"""
    group = blz.LoopGroup(nranks)
    said = [None] * nranks

    def rank_main(g):
        with blz.Context(p, n) as ctx:
            ctx.comm_init_loopback(group, g)
            prepare(ctx, g)
            with pytest.raises(blz.BlzError) as e:
                call(ctx, g)
            assert e.value.code == blz.EINVAL, str(e.value)
            said[g] = str(e.value)

    try:
        run_ranks(nranks, rank_main)
    finally:
        group.close()
    assert any(all(f in s for f in fragments) for s in said), said
    assert all(all(f in s for f in fragments) or "another rank" in s for s in said), said
    return said


def test_what_is_refused_on_several_ranks_is_refused_by_every_rank():
    p, n, nranks = P61, 4, 3
    Mb, Mx = pair("rand300x200", p)
    cols = RB.planted(Mx, True, p, 3, 31)[1]
    B = RB.rows(cols)
    L = blz.lib()
    nothing = lambda ctx, g: None                                           # noqa: E731
    bordered = blz.Matrix(Mb.nrows, Mb.ncols + 3, Mb.i, Mb.j, Mb.x)

    # external-exchange mode, before and after
    refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_exchange_mode(True),
                          lambda ctx, g: ctx.set_matrix_rhs_ranks(Mb, B, True, g, nranks), ["external-exchange"])

    def set_then_external(ctx, g):
        ctx.set_matrix(bordered, True, g, nranks)
        ctx.set_exchange_mode(True)

    refused_on_every_rank(nranks, p, n, set_then_external, lambda ctx, g: ctx.set_rhs_ranks(B), ["external-exchange"])
    refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_matrix_rhs_ranks(Mb, B, True, g, nranks),
                          lambda ctx, g: ctx.set_exchange_mode(True), ["right-hand side on several ranks"])
    # the last three columns of the matrix are not empty: the ranks that own them say so, the others learn it
    said = refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_matrix(Mb, True, g, nranks),
                                 lambda ctx, g: ctx.set_rhs_ranks(B), ["must be empty"])
    assert len(said) == nranks
    # two empty columns are one too few for three right-hand sides
    two = blz.Matrix(Mb.nrows, Mb.ncols + 2, Mb.i, Mb.j, Mb.x)
    refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_matrix(two, True, g, nranks),
                          lambda ctx, g: ctx.set_rhs_ranks(B), ["must be empty"])
    # a word equal to p
    bad = B.copy()
    bad[7, 2] = p
    refused_on_every_rank(nranks, p, n, nothing, lambda ctx, g: ctx.set_matrix_rhs_ranks(Mb, bad, True, g, nranks), ["not below p"])
    refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_matrix(bordered, True, g, nranks),
                          lambda ctx, g: ctx.set_rhs_ranks(bad), ["not below p"])
    # k = 0 and k = n + 1
    big = np.zeros(300 * 17, dtype=np.uint64)
    for k in (0, n + 1, 17):
        refused_on_every_rank(nranks, p, n, lambda ctx, g: ctx.set_matrix(bordered, True, g, nranks),
                              lambda ctx, g: blz.check(L.blz_set_rhs_ranks(ctx.h, C.c_int(k), blz.ptr(big))), ["right-hand sides"])
        refused_on_every_rank(nranks, p, n, nothing,
                              lambda ctx, g: blz.check(L.blz_set_matrix_rhs_ranks(ctx.h, C.byref(Mb.c), C.c_int(1), C.c_int(k),
                                                                                  blz.ptr(big), C.c_int(g), C.c_int(nranks))),
                              ["right-hand sides"])
    # and what the old entry points refuse stays refused, in their words
    refused_on_every_rank(nranks, p, n, nothing, lambda ctx, g: ctx.set_matrix_rhs_block(Mb, B, True), ["single rank"])
    # no matrix, no b
    with blz.Context(p, n) as ctx:
        with pytest.raises(blz.BlzError) as e:
            blz.check(L.blz_set_rhs_ranks(ctx.h, C.c_int(3), blz.ptr(B.reshape(-1))))
        assert e.value.code == blz.EINVAL and "no matrix" in str(e.value)
        # a plain single rank: blz_set_rhs_block in every respect, its refusals included
        ctx.set_matrix(Mb, True)
        with pytest.raises(blz.BlzError) as e:
            ctx.set_rhs_ranks(B)
        assert e.value.code == blz.EINVAL and "blz_set_rhs_block" in str(e.value) and "must be empty" in str(e.value)
        ctx.set_matrix_rhs_ranks(Mb, B, True, 0, 1)
        assert ctx.rhs_count == 3 and ctx.rows(blz.V) == 203
        ctx.init_v()
        while not ctx.iterate(16)[1]:
            pass
        status, x = ctx.solution_block()
    ref = one_rank("rand300x200", p, n, True, ("planted", 3, 31))
    assert status == ref[0] and np.array_equal(x, ref[1])
    # several ranks asked of a context without a communicator
    with blz.Context(p, n) as ctx:
        with pytest.raises(blz.BlzError) as e:
            ctx.set_matrix_rhs_ranks(Mb, B, True, 0, 2)
        assert e.value.code == blz.ECOMM


@pytest.mark.parametrize("nranks", (2, 3))
def test_a_bordered_context_runs_no_short_side_product(monkeypatch, nranks):
    """9000 x 400, x M = B: a plain several-rank context runs the product over the long side in its short-side form, and
    blz_set_rhs_ranks refuses that matrix in so many words; the one-call form plans none, whatever BLZ_SHORT_SIDE says, and
    solves: statuses and x those of the one-rank context, residuals zero."""
    p, n, k = P61, 8, 2
    Mb = blz.Matrix.synth(9000, 400, 90000, 0x4C4F4F50, p)
    Mx = X.Coo(Mb.nrows, Mb.ncols, ints(Mb.i), ints(Mb.j), ints(Mb.x))
    cols = RB.planted(Mx, False, p, k, 81)[1]
    B = RB.rows(cols)
    bordered = blz.Matrix(Mb.nrows + k, Mb.ncols, Mb.i, Mb.j, Mb.x)

    def short_side_on(ctx, g):
        ctx.set_matrix(bordered, False, g, nranks)
        assert (ctx.short_side(False), ctx.short_side(True)).count(True) == 1

    said = refused_on_every_rank(nranks, p, n, short_side_on, lambda ctx, g: ctx.set_rhs_ranks(B), ["short-side form"])
    assert all("not gathered" in s for s in said)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix_rhs_block(Mb, B, False)
        ctx.init_v()
        while not ctx.iterate(32)[1]:
            pass
        one_status, one_x = ctx.solution_block()
        one_its = ctx.iterations
    for forced in (None, "1"):
        if forced:
            monkeypatch.setenv("BLZ_SHORT_SIDE", forced)
        got = solve_on_ranks(Mb, cols, p, n, False, nranks, batch=32)
        for q in got:
            assert q["short"] == (False, False) and q["fused"] == [0, 0]
            assert q["status"] == one_status and q["its"] == one_its
        x = merged_x(got, Mx.nrows, k)
        assert np.array_equal(x, one_x)
    for i, (xi, b) in enumerate(zip(RB.columns(x), cols)):
        if one_status[i] == 0:
            assert not any(R.residual(Mx, xi, b, False, p)), i
    assert 0 in one_status


# ------------------------------------------------------------------------------------------------- F. the command line


def cli(args, cwd=None, loopback=True):
    env = dict(os.environ, BLZ_LOOPBACK="1") if loopback else dict(os.environ)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, timeout=300, env=env)


def solve_lines(r):
    lines = r.stdout.replace("\r", "\n").split("\n")
    at = lines.index("Solve:")
    return [ln for ln in lines[at:] if ln.startswith("Solve:") or ln.startswith("  - ") or ln.startswith("Saving") or ln.startswith("Not saving")]


@pytest.mark.parametrize("n,k,seed", ((4, 1, 41), (8, 3, 51)))
def test_cli_rhs_gpus_writes_what_the_one_rank_run_writes(tmp_path, n, k, seed):
    p, name = 65537, "rand300x200"
    Mx = pair(name, p)[1]
    x0s, cols = RB.planted(Mx, True, p, k, seed)
    assert all(verdict(name, p, n, True, ("planted", k, seed))["solvable"])
    local = str(tmp_path / "m.mtx")
    shutil.copy(mpath(name), local)
    bpath = RB.write_block(tmp_path / "b.mtx", cols, p)
    base = ["--matrix", local, "--prime", str(p), "--n", str(n), "--right", "--rhs", bpath]
    out1, out3, out3c, out2 = (str(tmp_path / f) for f in ("x1.mtx", "x3.mtx", "x3c.mtx", "x2.mtx"))
    plain = cli(base + ["--output-file", out1], loopback=False)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    r = cli(base + ["--rhs-gpus", "3", "--output-file", out3])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loopback communicator" in r.stderr
    assert [ln.replace(out3, out1) for ln in solve_lines(r)] == solve_lines(plain)
    assert open(out1, "rb").read() == open(out3, "rb").read()
    ref = str(tmp_path / "x0.mtx")                      # the only solutions: the file is the planted block's
    blz.save_block(ref, len(x0s[0]), k, RB.rows(x0s).reshape(-1))
    assert open(ref, "rb").read() == open(out3, "rb").read()
    chk = subprocess.run([CHECKER, "--matrix", local, "--kernel", out3, "--rhs", bpath, "--prime", str(p), "--right"],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and chk.stdout.splitlines()[1:] == ["OK"] * k, chk.stdout + chk.stderr
    # --cache, keyed by the rank count: written, mapped by the second run, not shared with another count
    for run, (gpus, mapped, files) in enumerate(((3, False, 1), (3, True, 1), (2, False, 2))):
        out = out3c if gpus == 3 else out2
        r = cli(base + ["--cache", "--verify", "--rhs-gpus", str(gpus), "--output-file", out])
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("mapped from" in r.stderr) == mapped, (run, r.stderr[-800:])
        assert len([f for f in os.listdir(tmp_path) if f.endswith(".blzcache")]) == files, run
        assert open(out1, "rb").read() == open(out, "rb").read(), run


def test_cli_rhs_gpus_checkpoint_written_by_three_ranks_resumed_by_two_and_by_one(tmp_path):
    p, n, k = 1073741789, 8, 4
    Mx = pair("rand3000x2000", p)[1]
    bpath = RB.write_block(tmp_path / "b.mtx", RB.planted(Mx, True, p, k, 44)[1], p)
    base = ["--matrix", mpath("rand3000x2000"), "--prime", str(p), "--n", str(n), "--right", "--rhs", bpath]
    full = str(tmp_path / "full.mtx")
    plain = cli(base + ["--output-file", full], loopback=False)
    assert plain.returncode == 0 and f"  - {k} of {k} systems solved\n" in plain.stdout, plain.stdout + plain.stderr
    work = tmp_path / "ck"
    work.mkdir()
    ck = str(tmp_path / "x3.mtx")
    r = cli(base + ["--rhs-gpus", "3", "--checkpoint", "0", "--output-file", ck], cwd=str(work))
    assert r.returncode == 0 and os.path.exists(work / "lanczos_modp.ckpt"), r.stdout + r.stderr
    assert open(full, "rb").read() == open(ck, "rb").read()
    saved = open(work / "lanczos_modp.ckpt", "rb").read()
    for gpus in (2, 1):
        open(work / "lanczos_modp.ckpt", "wb").write(saved)
        out = str(tmp_path / f"resumed{gpus}.mtx")
        r = cli(base + ["--load-checkpoint", "--output-file", out] + (["--rhs-gpus", str(gpus)] if gpus > 1 else []), cwd=str(work),
                loopback=gpus > 1)
        assert r.returncode == 0 and f"  - {k} of {k} systems solved\n" in r.stdout, r.stdout + r.stderr
        assert open(full, "rb").read() == open(out, "rb").read(), gpus


def test_cli_rhs_gpus_on_a_tall_matrix_plans_no_short_side_product(tmp_path):
    """9000 x 400, x M = B at 2^61 - 1: a plain --gpus 2 run of this shape takes the short-side form, which a bordered context
    cannot use; --rhs-gpus plans none and writes what the one-rank run writes."""
    p, n, k = P61, 8, 2
    Mb = blz.Matrix.synth(9000, 400, 90000, 0x4C4F4F50, p)
    local = str(tmp_path / "tall.mtx")
    Mb.save(local)
    Mx = X.load_mtx(local, p)
    cols = RB.planted(Mx, False, p, k, 81)[1]
    bpath = RB.write_block(tmp_path / "b.mtx", cols, p)
    base = ["--matrix", local, "--prime", str(p), "--n", str(n), "--left", "--rhs", bpath]
    one, two = str(tmp_path / "x1.mtx"), str(tmp_path / "x2.mtx")
    plain = cli(base + ["--output-file", one], loopback=False)
    assert plain.returncode == 0 and "systems solved" in plain.stdout, plain.stdout + plain.stderr
    r = cli(base + ["--rhs-gpus", "2", "--cache", "--output-file", two])
    assert r.returncode == 0, r.stdout + r.stderr
    assert [ln.replace(two, one) for ln in solve_lines(r)] == solve_lines(plain)
    if os.path.exists(one):
        assert open(one, "rb").read() == open(two, "rb").read()
        chk = subprocess.run([CHECKER, "--matrix", local, "--kernel", two, "--rhs", bpath, "--prime", str(p), "--left"],
                             capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout + chk.stderr
    assert os.path.exists(one) and os.path.exists(two)


def test_cli_rhs_gpus_exclusions(tmp_path):
    p = 65537
    Mx = pair("rand300x200", p)[1]
    bpath = RB.write_block(tmp_path / "b.mtx", RB.planted(Mx, True, p, 1, 43)[1], p)
    base = ["--matrix", mpath("rand300x200"), "--prime", str(p), "--n", "4", "--right"]
    for args in (base + ["--rhs-gpus", "2"], base + ["--rhs", bpath, "--rhs-gpus", "2", "--gpus", "2"], base + ["--rhs", bpath, "--gpus", "2"]):
        r = cli(args)
        assert r.returncode == 0 and "Options:" in r.stdout and "--rhs-gpus G" in r.stdout, args
        assert "Loading matrix" not in r.stdout and "Solve:" not in r.stdout
    for value in ("0", "-1", "65", "two"):              # not a count of GPUs: an error, not a silent one-rank run
        r = cli(base + ["--rhs", bpath, "--rhs-gpus", value])
        assert r.returncode == 1 and "--rhs-gpus must be between 1 and 64" in r.stderr, value
        assert "Solve:" not in r.stdout
