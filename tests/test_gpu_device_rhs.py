"""Device right-hand sides on the GPU: blz_set_rhs_device / blz_solution_device and their 32-bit twins (csrc/blz_devrhs.hip).

1. the import kernel: after set_rhs_device both products through blz_spmv equal exact integers on the augmented matrix
   (rhs_block_ref) AND, word for word, a twin context set with set_rhs_block -- every kp instantiation, every width of
   widths(k), one prime per reducer class, random and all-(p-1) operands, ldb = k and k + 3, a view that starts one word
   into its allocation, with the default renumbering and on a device-built matrix (no permutation), the grid-stride tail on
   rand3000x2000, and the 32-bit twin with words >= 2^31 in an int32 tensor;
2. whole solves, device end to end, against a host twin word for word, against the planted solutions, and against a plain
   context's apply; mixed, all-inconsistent, k = 1 and ldx > k;
3. every refusal by name, with b untouched and the resident border still applying;
4. the state a second call and a new matrix leave.

Every comparison is equality of words.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import blz
import exact_ref as X
import rhs_block_ref as RB
import rhs_ref as R
from test_gpu_rhs_block import PRIMES, SOLVE_SHAPES, mpath, operands, pair, widths

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P31, P61 = X.P31, X.P61
KS = (1, 2, 3, 5, 8, 16)                # kp = 0 (the single border), 2, 4, 8 (padded), 8, 16
KINDS = ("random", "max")
ALL_ONES64, ALL_ONES32 = (1 << 64) - 1, (1 << 32) - 1


def dev_rhs(B, ld=None, bits=64):
    """(tensor, its allocation) of the len x k block B on the GPU as a signed tensor of `bits` bits: contiguous when ld is
    None; otherwise a view of row stride ld that starts ONE word into its allocation, every word outside the k columns all ones
    (not below any p: a kernel that read one would count it)."""
    udt, sdt = (np.uint64, np.int64) if bits == 64 else (np.uint32, np.int32)
    B = np.ascontiguousarray(B, dtype=udt)
    rows, k = B.shape if B.ndim == 2 else (B.shape[0], 1)       # (a 1-D B: one right-hand side as a (rows,) tensor)
    if ld is None:
        t = torch.from_numpy(B.view(sdt).copy()).to(DEV)
        return t, t
    flat = np.full(1 + rows * ld, ALL_ONES64 if bits == 64 else ALL_ONES32, dtype=udt)
    flat[1:].reshape(rows, ld)[:, :k] = B
    alloc = torch.from_numpy(flat.view(sdt)).to(DEV)
    return alloc[1:].view(rows, ld)[:, :k], alloc


def bordered(M, right, k):
    return blz.Matrix(M.nrows + (0 if right else k), M.ncols + (k if right else 0), M.i, M.j, M.x)


def both_products(ctx, right, v, t):
    """(tmp after the product that carries the border update, av after the one that carries the border dot) as int lists"""
    ctx.set_block(blz.V, R.as_u64(v))
    ctx.spmv(not right, blz.V, blz.TMP)
    tmp = [int(w) for w in ctx.get_block(blz.TMP)]
    ctx.set_block(blz.TMP, R.as_u64(t))
    ctx.spmv(right, blz.TMP, blz.AV)
    return tmp, [int(w) for w in ctx.get_block(blz.AV)]


def host_twin_products(Mb, p, n, right, cols, v, t, built):
    with blz.Context(p, n) as twin:
        (twin.set_matrix_upload if built else twin.set_matrix)(Mb, right)
        twin.set_rhs_block(RB.rows(cols))
        return both_products(twin, right, v, t)


# ------------------------------------------------------------------------------------------------- 1. the import kernel


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", PRIMES)
def test_the_imported_border_is_exact_and_the_host_calls_word_for_word(p, right, k):
    Mb, Mx = pair("quirks40x30", p)
    Mk = bordered(Mb, right, k)
    for n in widths(k):
        for s, kind in enumerate(KINDS):
            cols, v, t = operands(kind, Mx, right, n, p, k, 1000 * n + 10 * k + s)
            A = RB.augmented(Mx, cols, right)
            want = (X.spmv(A, v, not right, n, p), X.spmv(A, t, right, n, p))
            B = RB.rows(cols)
            for built in (False, True):         # the default renumbering, and a device-built matrix: no permutation
                assert host_twin_products(Mk, p, n, right, cols, v, t, built) == want, (n, kind, built, "host twin")
                with blz.Context(p, n) as ctx:
                    (ctx.set_matrix_upload if built else ctx.set_matrix)(Mk, right)
                    assert ctx.matrix_device_built() == built and ctx.rhs_count == 0
                    for ld in (None, k + 3):
                        tb, alloc = dev_rhs(B if k > 1 or ld else B[:, 0], ld)
                        keep = alloc.clone()
                        ctx.set_rhs_device(tb)
                        assert ctx.has_rhs and ctx.rhs_count == k
                        assert both_products(ctx, right, v, t) == want, (n, kind, built, ld)
                        for tr in (False, True):
                            assert ctx.plan(tr)["fused"] == 0
                        assert torch.equal(alloc, keep)
                        ctx.set_rhs_device(dev_rhs(np.zeros_like(B), None)[0])      # (the next layout starts from another border)


def test_the_grid_stride_tail_runs_on_a_length_that_is_no_multiple_of_the_workgroup():
    p, n, k, right = P61, 8, 3, True
    Mb, Mx = pair("rand3000x2000", p)
    Mk = bordered(Mb, right, k)
    cols, v, t = operands("random", Mx, right, n, p, k, 7)
    assert len(cols[0]) == 3000 and (3000 * 4) % 256 != 0          # kp = 4 words per row of the border
    A = RB.augmented(Mx, cols, right)
    want = (X.spmv(A, v, not right, n, p), X.spmv(A, t, right, n, p))
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(Mk, right)
        ids = ctx.local_row_ids(blz.TMP)
        assert not np.array_equal(ids, np.arange(len(ids))), "the default numbering is the identity: the gather is not exercised"
        tb, alloc = dev_rhs(RB.rows(cols), k + 3)
        ctx.set_rhs_device(tb)
        assert both_products(ctx, right, v, t) == want


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (65537, P31, 4294967291))
def test_the_32_bit_twin_imports_the_same_border(p, right):
    Mb, Mx = pair("quirks40x30", p)
    for k, n in ((1, 8), (2, 2), (3, 8), (5, 16), (8, 8), (16, 64)):
        Mk = bordered(Mb, right, k)
        for s, kind in enumerate(KINDS):
            cols, v, t = operands(kind, Mx, right, n, p, k, 500 * n + 10 * k + s)
            want = host_twin_products(Mk, p, n, right, cols, v, t, False)
            B = RB.rows(cols)
            if kind == "max" and p > 1 << 31:
                assert int(B.max()) >= 1 << 31      # negative as int32: the same 32 bits
            for built in (False, True):
                with blz.Context(p, n) as ctx:
                    assert ctx.word_bytes == 4
                    (ctx.set_matrix_upload if built else ctx.set_matrix)(Mk, right)
                    for ld in (None, k + 3):
                        tb, alloc = dev_rhs(B if k > 1 or ld else B[:, 0], ld, bits=32)
                        assert tb.dtype == torch.int32
                        keep = alloc.clone()
                        ctx.set_rhs_device32(tb)
                        assert ctx.rhs_count == k and both_products(ctx, right, v, t) == want, (k, n, kind, built, ld)
                        assert torch.equal(alloc, keep)


# ------------------------------------------------------------------------------------------------- 2. whole solves


def triplets(M):
    return (torch.from_numpy(np.ascontiguousarray(M.i, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(M.j, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(M.x, dtype=np.uint32).view(np.int32)).to(DEV))


def words(t):
    """a device tensor of 64-bit words as numpy u64"""
    torch.cuda.synchronize()
    return t.cpu().contiguous().numpy().view(np.uint64)


def run_to_the_stop(ctx):
    ctx.init_v()
    while not ctx.iterate(16)[1]:
        pass
    return ctx.iterations


def solve_both_ways(Mb, cols, p, n, right, out=None):
    """the host solve and the device solve of the same systems on a twin pair of contexts; every word they leave is compared
    here, and (statuses, x of the device solve as a tensor, iterations, b on the device) come back"""
    k = len(cols)
    B = RB.rows(cols)
    with blz.Context(p, n) as host, blz.Context(p, n) as dev:
        host.set_matrix_rhs_block(Mb, B, right)
        i, j, x = triplets(Mb)
        tb, _ = dev_rhs(B)
        keep = tb.clone()
        dev.set_matrix_rhs_device(i, j, x, tb, Mb.nrows, Mb.ncols, right)
        assert dev.matrix_device_built() and dev.rhs_count == k == host.rhs_count
        assert dev.rows(blz.V) == host.rows(blz.V) and dev.rows(blz.TMP) == host.rows(blz.TMP) == B.shape[0]
        its = (run_to_the_stop(host), run_to_the_stop(dev))
        assert its[0] == its[1]
        for blk in (blz.V, blz.P, blz.TMP):
            assert np.array_equal(host.get_block(blk), dev.get_block(blk)), blk
        hs, hx = host.solution_block()
        ds, dx = dev.solution_device(out=out)
        assert hs == ds and torch.equal(tb, keep)
        got = words(dx)
        if 2 not in hs:
            assert got.shape == hx.shape == (dev.rows(blz.V) - k, k) and np.array_equal(got, hx)
        for blk in (blz.V, blz.TMP):
            assert np.array_equal(host.get_block(blk), dev.get_block(blk)), ("after the solution", blk)
        return ds, dx, its[1], tb


@pytest.mark.parametrize("p,n,k", SOLVE_SHAPES)
@pytest.mark.parametrize("name,right", (("rand300x200", True), ("wide120x260", False)))
def test_whole_solves_device_end_to_end(name, right, p, n, k):
    Mb, Mx = pair(name, p)
    x0s, cols = RB.planted(Mx, right, p, k, 51)
    ref = RB.verdict(Mx, cols, right, n, p)
    assert ref["w_rank"] == k and all(ref["solvable"])          # the restatement solves all k on the CPU: a miss is the GPU's
    status, x, its, tb = solve_both_ways(Mb, cols, p, n, right)
    assert status == [0] * k and its == ref["iterations"]
    assert x.dtype == torch.uint64 and x.device.type == "cuda"
    assert RB.columns(words(x)) == x0s
    with blz.Context(p, k) as plain:            # independently: M x = b (right) / x M = b on a plain context of width k
        plain.set_matrix(Mb, right)
        y = plain.apply(not right, x)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int64), tb)


def test_an_inconsistent_system_between_two_planted_ones_gives_a_zero_column():
    p, n = 65537, 8
    Mb, Mx = pair("rand300x200", p)
    x0s, cols = RB.planted(Mx, True, p, 3, 53)
    cols[1] = R.random_rhs(Mx, True, p, 53)
    ref = RB.verdict(Mx, cols, True, n, p)
    assert ref["solvable"] == [1, 0, 1] and ref["w_rank"] == 2
    status, x, its, _ = solve_both_ways(Mb, cols, p, n, True)
    assert status == [0, 1, 0] and its == ref["iterations"]
    got = RB.columns(words(x))
    assert got[0] == x0s[0] and got[2] == x0s[2] and not any(got[1])


def test_inconsistent_systems_give_an_x_of_zeros():
    p, n, k = 65537, 8, 3
    Mb, Mx = pair("rand300x200", p)
    cols = [R.random_rhs(Mx, True, p, 54 + i) for i in range(k)]
    assert RB.verdict(Mx, cols, True, n, p)["solvable"] == [0] * k
    out = torch.full((200, k), 7, dtype=torch.int64, device=DEV)        # every word is written, with zeros
    status, x, _, _ = solve_both_ways(Mb, cols, p, n, True, out=out)
    assert status == [1] * k and x is out and not words(x).any()


@pytest.mark.parametrize("name,right,p,n", (("rand300x200", True, P61, 4), ("wide120x260", False, 65537, 8)))
def test_one_right_hand_side_is_the_single_solve(name, right, p, n):
    Mb, Mx = pair(name, p)
    x0, b = R.planted(Mx, right, p, 61)
    with blz.Context(p, n) as host, blz.Context(p, n) as dev:
        host.set_matrix_rhs(Mb, R.as_u64(b), right)
        i, j, x = triplets(Mb)
        dev.set_matrix_rhs_device(i, j, x, dev_rhs(RB.rows([b])[:, 0])[0], Mb.nrows, Mb.ncols, right)      # a 1-D tensor
        assert dev.rhs_count == 1 and run_to_the_stop(host) == run_to_the_stop(dev)
        hs, hx = host.solution()
        ds, dx = dev.solution_device()
        assert hs == 0 and ds == [0] and dx.shape == (len(x0), 1)
        assert np.array_equal(words(dx)[:, 0], hx) and not any(R.residual(Mx, hx, b, right, p))
        for blk in (blz.V, blz.TMP):
            assert np.array_equal(host.get_block(blk), dev.get_block(blk)), blk


@pytest.mark.parametrize("bits,p", ((64, P61), (64, 65537), (32, 65537), (32, 4294967291)))
def test_words_past_k_of_a_row_of_x_keep_their_sentinel(bits, p):
    n, k, right = 8, 3, True
    Mb, Mx = pair("rand300x200", p)
    x0s, cols = RB.planted(Mx, right, p, k, 51)
    B = RB.rows(cols)
    sdt, udt = (torch.int64, np.uint64) if bits == 64 else (torch.int32, np.uint32)
    sentinel = 0x5A5A5A5A
    with blz.Context(p, n) as ctx:
        i, j, x = triplets(Mb)
        ctx.set_matrix_device(i, j, x, Mb.nrows, Mb.ncols + k, right)
        if bits == 64:
            ctx.set_rhs_device(dev_rhs(B)[0])
        else:
            ctx.set_rhs_device32(dev_rhs(B, bits=32)[0])
        run_to_the_stop(ctx)
        wide = torch.full((200, k + 2), sentinel, dtype=sdt, device=DEV)
        status, out = (ctx.solution_device if bits == 64 else ctx.solution_device32)(out=wide[:, :k])
        torch.cuda.synchronize()
        assert status == [0] * k and out.stride() == (k + 2, 1)
        got = wide.cpu().numpy().view(udt)
        assert (got[:, k:] == sentinel).all()
        # (solutions, not THE solutions: modulo 2^32 - 5 this matrix has a kernel and the planted x0 is one of several)
        for xi, b in zip(RB.columns(got[:, :k]), cols):
            assert not any(R.residual(Mx, xi, b, right, p))


def guarded_x(rows, k, bits, guard=64, sentinel=0x5A5A5A5A):
    """(x, its allocation): a (rows, k) view of row stride k + 2 in the MIDDLE of an allocation of sentinels, `guard` rows of
    them before and behind: a row written to the wrong place, or past the end of x, shows"""
    alloc = torch.full((rows + 2 * guard, k + 2), sentinel, dtype=torch.int64 if bits == 64 else torch.int32, device=DEV)
    return alloc[guard:guard + rows, :k], alloc


def outside_is_untouched(alloc, rows, k, bits, guard=64, sentinel=0x5A5A5A5A):
    torch.cuda.synchronize()
    got = alloc.cpu().numpy().view(np.uint64 if bits == 64 else np.uint32)
    return bool((got[:guard] == sentinel).all() and (got[guard + rows:] == sentinel).all() and (got[:, k:] == sentinel).all())


def renumbered_solution(Mb, cols, p, n, right, bits):
    """solution_device / solution_device32 out of a RENUMBERED slab (the matrix set on the host, the default numbering) into a
    guarded x, against the host twin's solution_block: (statuses, x as numpy, the host's x)"""
    k = len(cols)
    B = RB.rows(cols)
    with blz.Context(p, n) as host, blz.Context(p, n) as dev:
        host.set_matrix_rhs_block(Mb, B, right)
        dev.set_matrix(bordered(Mb, right, k), right)
        assert not dev.matrix_device_built()
        ids = dev.local_row_ids(blz.V)
        assert not np.array_equal(ids, np.arange(len(ids))), "the numbering of V's side is the identity: the scatter is not exercised"
        if bits == 64:
            dev.set_rhs_device(dev_rhs(B, k + 3)[0])
        else:
            dev.set_rhs_device32(dev_rhs(B, k + 3, bits=32)[0])
        assert run_to_the_stop(host) == run_to_the_stop(dev)
        hs, hx = host.solution_block()
        rows = dev.rows(blz.V) - k
        x, alloc = guarded_x(rows, k, bits)
        ds, out = (dev.solution_device if bits == 64 else dev.solution_device32)(out=x)
        assert out is x and ds == hs and outside_is_untouched(alloc, rows, k, bits)
        got = x.cpu().numpy().view(np.uint64 if bits == 64 else np.uint32).astype(np.uint64)
        assert got.shape == hx.shape and np.array_equal(got, hx)
        for blk in (blz.V, blz.TMP):
            assert np.array_equal(host.get_block(blk), dev.get_block(blk)), ("after the solution", blk)
        return ds, got, hx


@pytest.mark.parametrize("p,n,k,bits", ((65537, 8, 3, 64), (65537, 8, 3, 32), (P61, 8, 5, 64), (P31, 16, 16, 32), (P31, 16, 16, 64)))
@pytest.mark.parametrize("name,right", (("rand300x200", True), ("wide120x260", False)))
def test_the_solution_leaves_a_renumbered_slab_row_by_row(name, right, p, n, k, bits):
    Mb, Mx = pair(name, p)
    x0s, cols = RB.planted(Mx, right, p, k, 51)
    status, got, _ = renumbered_solution(Mb, cols, p, n, right, bits)
    assert status == [0] * k
    assert RB.columns(got) == x0s


def test_the_solution_leaves_the_renumbered_slab_of_the_large_matrix():
    """rand3000x2000: more rows than one pass of the grid's first workgroups; the solutions are not the only ones there, so
    they are compared with the host twin's and by their residuals"""
    c = RB.RECORDED_CASE
    p, n, k, right = c["p"], c["n"], c["k"], c["right"]
    Mb, Mx = pair(c["name"], p)
    cols = RB.planted(Mx, right, p, k, c["seed"])[1]
    assert all(RB.recorded()["solvable"])
    status, got, _ = renumbered_solution(Mb, cols, p, n, right, 64)
    assert status == [0] * k
    for xi, b in zip(RB.columns(got), cols):
        assert not any(R.residual(Mx, xi, b, right, p))


def sparse_tensor(M):
    idx = torch.from_numpy(np.stack([np.asarray(M.i, dtype=np.int64), np.asarray(M.j, dtype=np.int64)])).to(DEV)
    val = torch.from_numpy(np.ascontiguousarray(M.x, dtype=np.uint32).astype(np.int64)).to(DEV)
    return torch.sparse_coo_tensor(idx, val, (M.nrows, M.ncols), device=DEV)


@pytest.mark.parametrize("name,right,p,n,k", (("rand300x200", True, 65537, 8, 3), ("wide120x260", False, P61, 8, 5)))
def test_solve_rhs_device_from_a_sparse_tensor_and_from_triplets(name, right, p, n, k):
    Mb, Mx = pair(name, p)
    x0s, cols = RB.planted(Mx, right, p, k, 51)
    ref = RB.verdict(Mx, cols, right, n, p)
    assert all(ref["solvable"])
    tb = dev_rhs(RB.rows(cols))[0]
    i, j, x = triplets(Mb)
    forms = [sparse_tensor(Mb), (i, j, x, Mb.nrows, Mb.ncols)]
    if int(Mb.i.max()) + 1 == Mb.nrows and int(Mb.j.max()) + 1 == Mb.ncols:         # only then may the dimensions be left out
        forms.append((i, j, x))
    assert len(forms) == 3 or name != "rand300x200"                                 # (wide120x260's last column is empty)
    for what in forms:
        got = blz.solve_rhs_device(what, tb, p, n, right=right)
        assert got["status"] == [0] * k and got["iterations"] == ref["iterations"] and len(got["final_check"]) == 2
        assert got["x"].dtype == torch.uint64 and got["x"].device.type == "cuda"
        assert RB.columns(words(got["x"])) == x0s
    # one right-hand side as a (rows,) tensor
    assert RB.verdict(Mx, cols[:1], right, n, p)["solvable"] == [1]
    got = blz.solve_rhs_device((i, j, x, Mb.nrows, Mb.ncols), dev_rhs(RB.rows(cols[:1])[:, 0])[0], p, n, right=right)
    assert got["status"] == [0] and RB.columns(words(got["x"])) == x0s[:1]
    with pytest.raises(ValueError, match="dimensions"):
        blz.solve_rhs_device(torch.zeros((2, 2, 2), device=DEV).to_sparse(), tb, p, n, right=right)


# ------------------------------------------------------------------------------------------------- 3. refusals


def refused(rc, *fragments):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL and all(f in msg for f in fragments), (rc, msg)


def raw_set(ctx, k, ptr_, ld, stream=0, fn="blz_set_rhs_device"):
    return getattr(blz.lib(), fn)(ctx.h, C.c_int(k), C.c_void_p(ptr_), C.c_int64(ld), C.c_void_p(stream))


def raw_solution(ctx, ptr_, ld, stream=0, fn="blz_solution_device"):
    return getattr(blz.lib(), fn)(ctx.h, C.c_void_p(ptr_), C.c_int64(ld), (C.c_int * 16)(), C.c_void_p(stream))


def test_every_refusal_names_its_argument_and_leaves_the_context_alone(monkeypatch):
    p, n, k = P61, 4, 3
    Mb, Mx = pair("rand300x200", p)
    Mk = bordered(Mb, True, k)
    cols, v, t = operands("random", Mx, True, n, p, k, 31)
    B = RB.rows(cols)
    tb, _ = dev_rhs(B)
    keep = tb.clone()
    pb = tb.data_ptr()
    xout = torch.zeros((200, k), dtype=torch.int64, device=DEV)
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    with blz.Context(p, n) as ctx:
        refused(raw_set(ctx, k, pb, k), "no matrix")
        refused(raw_solution(ctx, xout.data_ptr(), k), "no matrix")
        ctx.set_matrix(Mk, True)
        refused(raw_solution(ctx, xout.data_ptr(), k), "blz_solution_device", "no right-hand side")
        with pytest.raises(ValueError, match="no right-hand side"):
            ctx.solution_device()
        for bad_k in (0, -1, 5, 17):                    # k < 1, k > n = 4, k > BLZ_MAX_RHS
            refused(raw_set(ctx, bad_k, pb, 17), "blz_set_rhs_device", "right-hand sides")
        refused(raw_set(ctx, k, pb, k - 1), "row stride of b", "less than k = 3")     # (k, not the block width n = 4)
        refused(raw_set(ctx, k, None, k), "b is NULL")
        refused(raw_set(ctx, k, B.ctypes.data, k), "b =", "not device memory")
        short = C.c_void_p()                            # one word short: an allocation of exactly 299 * k + k - 1 words
        assert hip.hipMalloc(C.byref(short), C.c_size_t((299 * k + k - 1) * 8)) == 0
        try:
            refused(raw_set(ctx, k, short.value, k), "b needs", "k = 3", "allocation ends")
            refused(raw_set(ctx, 2, short.value, k + 1), "b needs", "allocation ends")      # and by its stride alone
        finally:
            assert hip.hipFree(short) == 0
        refused(raw_set(ctx, k, pb + 4, k), "b is not aligned")
        refused(raw_set(ctx, k, pb, k, fn="blz_set_rhs_device32"), "blz_set_rhs_device32", "32-bit")    # p >= 2^32
        s, g = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):             # captured and thrown away: never replayed
            got = raw_set(ctx, k, pb, k, torch.cuda.current_stream().cuda_stream)
            msg = blz.lib().blz_last_error().decode()
            xout.add_(0)                                # (a graph of one node, not an empty one)
        torch.cuda.synchronize()
        assert got == blz.EINVAL and "capturing" in msg, (got, msg)
        assert ctx.rhs_count == 0 and not ctx.has_rhs
        ctx.set_matrix(Mb, True)                        # one rank, but the last three columns are not empty
        refused(raw_set(ctx, k, pb, k), "must be empty")
        ctx.set_matrix(bordered(Mb, True, 2), True)     # two empty columns are one too few
        refused(raw_set(ctx, k, pb, k), "must be empty")
        ctx.set_matrix(Mk, True, rank=0, nranks=2)      # two ranks (external exchange)
        refused(raw_set(ctx, k, pb, k), "single rank")
        ctx.set_matrix(Mk, True)
        ctx.device_ranks(True)
        refused(raw_set(ctx, k, pb, k), "blz_set_device_ranks")
        ctx.device_ranks(False)

        # one word equal to p: refused with the count, and the border set before still applies
        ctx.set_rhs_device(tb)
        before = both_products(ctx, True, v, t)
        bad = B.copy()
        bad[7, 2] = p
        tbad, _ = dev_rhs(bad, k + 3)
        with pytest.raises(blz.BlzError) as e:
            ctx.set_rhs_device(tbad)
        assert e.value.code == blz.EINVAL and "1 words of b are not below p" in str(e.value), str(e.value)
        assert ctx.rhs_count == k and both_products(ctx, True, v, t) == before
        refused(raw_set(ctx, 2, pb, 1), "row stride of b")              # and so it does after a refusal by argument
        assert ctx.rhs_count == k and both_products(ctx, True, v, t) == before
        # the solution's own arguments (the state: a border, no solve -- nothing is reduced before they are refused)
        refused(raw_solution(ctx, xout.data_ptr(), k - 1), "row stride of x")
        refused(raw_solution(ctx, None, k), "x is NULL")
        short = C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t((199 * k + k - 1) * 8)) == 0
        try:
            refused(raw_solution(ctx, short.value, k), "x needs", "allocation ends")
        finally:
            assert hip.hipFree(short) == 0
        refused(raw_solution(ctx, xout.data_ptr() + 4, k), "x is not aligned")
        refused(raw_solution(ctx, xout.data_ptr(), k, fn="blz_solution_device32"), "blz_solution_device32", "32-bit")
        refused(blz.lib().blz_solution_device(ctx.h, C.c_void_p(xout.data_ptr()), C.c_int64(k), None, None), "status is NULL")
        ctx.device_ranks(True)
        refused(raw_solution(ctx, xout.data_ptr(), k), "blz_set_device_ranks")
        ctx.device_ranks(False)
        assert both_products(ctx, True, v, t) == before and not words(xout).any()
    assert torch.equal(tb, keep)

    # a loopback group of two, and one rank with the collectives forced on
    grp = blz.LoopGroup(2)
    try:
        with blz.Context(p, n) as c0, blz.Context(p, n) as c1:
            c0.comm_init_loopback(grp, 0)
            c1.comm_init_loopback(grp, 1)
            refused(raw_set(c0, k, pb, k), "single rank")
    finally:
        grp.close()
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")           # read when the communicator is attached
    one = blz.LoopGroup(1)
    try:
        with blz.Context(p, n) as ctx:
            ctx.comm_init_loopback(one, 0)
            refused(raw_set(ctx, k, pb, k), "single rank", "BLZ_FORCE_COMM")
    finally:
        one.close()
    assert torch.equal(tb, keep)


# ------------------------------------------------------------------------------------------------- 4. state


def test_a_second_call_replaces_the_border_and_a_new_matrix_drops_it():
    p, n = 65537, 8
    Mb, Mx = pair("quirks40x30", p)
    for right in (False, True):
        Mk = bordered(Mb, right, 5)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(Mk, right)
            for seed in (1, 2):
                cols, v, t = operands("random", Mx, right, n, p, 5, seed)
                ctx.set_rhs_device(dev_rhs(RB.rows(cols))[0])
                assert ctx.rhs_count == 5
                A = RB.augmented(Mx, cols, right)
                assert both_products(ctx, right, v, t) == (X.spmv(A, v, not right, n, p), X.spmv(A, t, right, n, p)), seed
            # a host border over a device one and back
            cols, v, t = operands("max", Mx, right, n, p, 5, 9)
            ctx.set_rhs_block(RB.rows(cols))
            want = both_products(ctx, right, v, t)
            ctx.set_rhs_device(dev_rhs(np.zeros((len(cols[0]), 5), dtype=np.uint64))[0])
            assert both_products(ctx, right, v, t) != want
            ctx.set_rhs_device(dev_rhs(RB.rows(cols), 8)[0])
            assert both_products(ctx, right, v, t) == want
            ctx.set_matrix(Mk, right)
            assert ctx.rhs_count == 0 and not ctx.has_rhs
            ctx.set_rhs_device(dev_rhs(RB.rows(cols))[0])
            ctx.set_matrix_upload(Mk, right)
            assert ctx.rhs_count == 0 and not ctx.has_rhs
