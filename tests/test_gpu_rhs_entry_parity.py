"""Every entry point that sets right-hand sides installs the same border, and blz_solution is blz_solution_block with k = 1.

The host setters (blz_set_rhs, blz_set_rhs_block, blz_set_rhs_ranks) and the device pair (blz_set_rhs_device[32]) end in
one install; this file holds them to each other on quirks40x30 and its bordered copies.  The truth is the augmented matrix
in Python integers (rhs_block_ref / rhs_ref / exact_ref), never the library:

1. every route, fresh context each: both products word for word, rhs_count, nothing fused;
2. transitions on one context, k = 1 -> 16 -> 1 and 3 -> 8 -> 2, host and device entries alternating: the scratch of the
   border dot and the row tables are sized for one border, then for sixteen, then for one again;
3. a host call that is refused leaves the resident border alone;
4. solution(), solution_block() and solution_device() on one right-hand side: equal status, x and V.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import blz
import exact_ref as X
import rhs_block_ref as RB
import rhs_ref as R
from test_gpu_device_rhs import both_products, bordered, dev_rhs
from test_gpu_rhs_block import mpath, operands

pytestmark = pytest.mark.gpu

P31, P61 = X.P31, X.P61
NAME = "quirks40x30"


@functools.lru_cache(maxsize=None)
def pair(p):
    return blz.Matrix.load(mpath(NAME), p), X.load_mtx(mpath(NAME), p)


def case(Mx, right, n, p, k, seed):
    """(the k x len block B, the operands v and t, the two products by the restatement)"""
    cols, v, t = operands("random", Mx, right, n, p, k, seed)
    A = RB.augmented(Mx, cols, right)
    return RB.rows(cols), v, t, (X.spmv(A, v, not right, n, p), X.spmv(A, t, right, n, p))


def one_column(B):
    return np.ascontiguousarray(B[:, 0])


def device_block(B, bits=64):
    return dev_rhs(B if B.shape[1] > 1 else one_column(B), None, bits)[0]


# how each entry point takes the block B (rows x k) on a context whose matrix is set
SETTERS = {
    "set_rhs": lambda ctx, B: ctx.set_rhs(one_column(B)),
    "set_rhs_block": lambda ctx, B: ctx.set_rhs_block(B),
    "set_rhs_ranks": lambda ctx, B: ctx.set_rhs_ranks(B),
    "set_rhs_device": lambda ctx, B: ctx.set_rhs_device(device_block(B)),
    "set_rhs_device32": lambda ctx, B: ctx.set_rhs_device32(device_block(B, 32)),
}


def installed(ctx, right, k, v, t, want, what):
    assert ctx.has_rhs and ctx.rhs_count == k, what
    assert both_products(ctx, right, v, t) == want, what
    assert [ctx.plan(tr)["fused"] for tr in (False, True)] == [0, 0], what


# ------------------------------------------------------------------------------------------------- 1. every route


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (65537, P61))
def test_every_route_installs_the_same_border(p, right):
    n = 8
    Mb, Mx = pair(p)
    for k in (1, 3, 8):
        Mk = bordered(Mb, right, k)
        B, v, t, want = case(Mx, right, n, p, k, 100 * k + right)
        routes = ["set_rhs"] * (k == 1) + ["set_rhs_block", "set_rhs_ranks", "set_rhs_device"] + ["set_rhs_device32"] * (p == 65537)
        for route in routes:
            with blz.Context(p, n) as ctx:
                ctx.set_matrix(Mk, right)
                assert ctx.rhs_count == 0
                SETTERS[route](ctx, B)
                installed(ctx, right, k, v, t, want, (k, route))
        group = blz.LoopGroup(1)            # blz_set_rhs_ranks proper: a one-rank loopback group is no plain context
        try:
            with blz.Context(p, n) as ctx:
                ctx.comm_init_loopback(group, 0)
                ctx.set_matrix(Mk, right, 0, 1)
                ctx.set_rhs_ranks(B)
                installed(ctx, right, k, v, t, want, (k, "set_rhs_ranks on a loopback group"))
        finally:
            group.close()


# ------------------------------------------------------------------------------------------------- 2. transitions

ONE = ("set_rhs", "set_rhs_block", "set_rhs", "set_rhs_ranks", "set_rhs", "set_rhs_device", "set_rhs_block", "set_rhs_device")
MANY = ("set_rhs_block", "set_rhs_device", "set_rhs_block", "set_rhs_ranks", "set_rhs_device")


@pytest.mark.parametrize("ks", ((1, 16, 1), (3, 8, 2)))
@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (65537, P61))
def test_transitions_between_the_entry_points_on_one_context(p, right, ks):
    """One context; the matrix is set once per k (the bordered shape depends on k) and the entries alternate on it, each with
    right-hand sides of its own.  set_rhs <-> set_rhs_block and set_rhs_ranks <-> set_rhs at k = 1, set_rhs_block <->
    set_rhs_device at every k."""
    n = 16
    Mb, Mx = pair(p)
    with blz.Context(p, n) as ctx:
        for at, k in enumerate(ks):
            ctx.set_matrix(bordered(Mb, right, k), right)
            assert ctx.rhs_count == 0
            for step, route in enumerate(ONE if k == 1 else MANY):
                B, v, t, want = case(Mx, right, n, p, k, 1000 * at + 10 * step + right)
                SETTERS[route](ctx, B)
                installed(ctx, right, k, v, t, want, (at, k, step, route))


# ------------------------------------------------------------------------------------------------- 3. refused host calls


def einval(rc, *fragments):
    msg = blz.lib().blz_last_error().decode()
    assert rc == blz.EINVAL and all(f in msg for f in fragments), (rc, msg)


def refused_host_calls(ctx, B, p, n):
    """(what it is, the call, a fragment of its message) for every host setter: a word equal to p, k = 0, k > n, b = NULL"""
    L = blz.lib()
    k = B.shape[1]
    bad = B.copy()
    bad[7, k - 1] = p
    bad1 = one_column(bad[:, k - 1:])
    big = np.zeros(B.shape[0] * (n + 1), dtype=np.uint64)
    calls = [("set_rhs: p", lambda: L.blz_set_rhs(ctx.h, blz.ptr(bad1)), "not below p"),
             ("set_rhs: NULL", lambda: L.blz_set_rhs(ctx.h, None), "b is NULL")]
    for name in ("blz_set_rhs_block", "blz_set_rhs_ranks"):
        fn = getattr(L, name)
        calls += [(name + ": p", lambda fn=fn: fn(ctx.h, C.c_int(k), blz.ptr(bad.reshape(-1))), "not below p"),
                  (name + ": k = 0", lambda fn=fn: fn(ctx.h, C.c_int(0), blz.ptr(big)), "right-hand sides"),
                  (name + ": k > n", lambda fn=fn: fn(ctx.h, C.c_int(n + 1), blz.ptr(big)), "right-hand sides"),
                  (name + ": NULL", lambda fn=fn: fn(ctx.h, C.c_int(k), None), "b is NULL")]
    return calls


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p", (65537, P61))
def test_a_refused_host_call_leaves_the_resident_border_alone(p, right):
    n, k = 8, 3
    Mb, Mx = pair(p)
    Mk = bordered(Mb, right, k)
    B, v, t, want = case(Mx, right, n, p, k, 300 + right)
    group = blz.LoopGroup(1)
    try:
        for loopback in (False, True):
            with blz.Context(p, n) as ctx:
                if loopback:            # blz_set_rhs_ranks proper; the one-rank setters refuse this context outright
                    ctx.comm_init_loopback(group, 0)
                    ctx.set_matrix(Mk, right, 0, 1)
                    ctx.set_rhs_ranks(B)
                else:
                    ctx.set_matrix(Mk, right)
                    ctx.set_rhs_block(B)
                installed(ctx, right, k, v, t, want, "before")
                for what, call, fragment in refused_host_calls(ctx, B, p, n):
                    if loopback and "ranks" not in what:
                        continue
                    einval(call(), fragment)
                    installed(ctx, right, k, v, t, want, (loopback, what))
                # the last five rows / columns hold two of the matrix's own, which are not empty
                five = np.zeros((B.shape[0], 5), dtype=np.uint64)
                with pytest.raises(blz.BlzError) as e:
                    (ctx.set_rhs_ranks if loopback else ctx.set_rhs_block)(five)
                assert e.value.code == blz.EINVAL and "must be empty" in str(e.value)
                installed(ctx, right, k, v, t, want, (loopback, "must be empty"))
                if not loopback:
                    with pytest.raises(blz.BlzError) as e:
                        ctx.set_rhs_ranks(five)
                    assert e.value.code == blz.EINVAL and "must be empty" in str(e.value)
                    installed(ctx, right, k, v, t, want, "must be empty, set_rhs_ranks on a plain context")
    finally:
        group.close()


# ------------------------------------------------------------------------------------------------- 4. one solution path


def to_the_stop(ctx):
    ctx.init_v()
    while not ctx.iterate(16)[1]:
        pass


def solved_three_ways(Mb, b, p, n, right):
    """[(status, x or None, V afterwards)] through solution(), solution_block() and solution_device(), the same run each"""
    out = []
    for way in ("solution", "solution_block", "solution_device"):
        with blz.Context(p, n) as ctx:
            ctx.set_matrix_rhs(Mb, R.as_u64(b), right)
            to_the_stop(ctx)
            if way == "solution":
                status, x = ctx.solution()
            elif way == "solution_block":
                st, x = ctx.solution_block()
                status, x = st[0], None if x is None else x[:, 0]
            else:
                st, x = ctx.solution_device()
                torch.cuda.synchronize()
                status, x = st[0], x.cpu().contiguous().numpy().view(np.uint64)[:, 0]
            out.append((status, None if x is None else [int(w) for w in x], ctx.get_block(blz.V).reshape(-1, n)))
    return out


@pytest.mark.parametrize("right", (False, True))
@pytest.mark.parametrize("p,n", ((P31, 1), (P61, 4)))
def test_solution_is_solution_block_with_one_right_hand_side(p, n, right):
    Mb, Mx = pair(p)
    rows = Mx.ncols if right else Mx.nrows
    # a planted system: solved, and the x every call gives solves it by the restatement
    _, b = R.planted(Mx, right, p, 22)
    one, block, device = solved_three_ways(Mb, b, p, n, right)
    assert one[0] == block[0] == device[0] == 0
    assert one[1] == block[1] == device[1] and len(one[1]) == rows
    assert not any(R.residual(Mx, one[1], b, right, p))
    assert np.array_equal(one[2], block[2]) and np.array_equal(one[2], device[2])
    V = one[2]
    assert [int(w) for w in V[:-1, 0]] == one[1] and int(V[-1, 0]) == p - 1 and not V[:, 1:].any()
    # an inconsistent one: not solved, by every call; blz_solution leaves x alone, the block calls a column of zeros
    b = R.random_rhs(Mx, right, p, 23)
    assert R.solve(Mx, b, right, p)[1] is None
    one, block, device = solved_three_ways(Mb, b, p, n, right)
    assert one[0] == block[0] == device[0] == 1
    assert one[1] is None and block[1] == device[1] == [0] * rows
    assert np.array_equal(one[2], block[2]) and np.array_equal(one[2], device[2])
