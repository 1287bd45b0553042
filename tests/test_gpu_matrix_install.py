"""One matrix install for the host upload and the device build (matrix_begin, csrc/blz_api.hip): a context that is given one
matrix after another keeps no trace of the one before, whichever of the two paths set either; and the stage-trace lines
of the device build are what tools/device_matrix_cost.py parses.

The installs of a context alternate between the paths and between left and right kernels.  After each one the context is
compared, field by field, with a fresh context that was given only that matrix by the same call, and one product per
orientation is compared with the CPU oracle.  Every comparison is equality of integers.

Step 5, "host in wide mode": blz_set_values_wide refuses a context that holds a matrix, and the device build refuses one with
high limbs pending, so the only install a host wide matrix can be is a context's first.  The 64-bit context therefore makes
nine installs: the host wide matrix in front of the eight, and at step 5 the device build of the same wide entries as 8-byte
values (the wide mode of the other path).  Wide to ordinary is then crossed on the host path (0 -> 1) and on the device path
(5 -> 6), ordinary to wide at 4 -> 5.  The 16-bit context (no residue has a high limb) makes the seven other installs.

Step 3, "host with BLZ_NO_REORDER=1": the library reads that variable when a context is created, so the resident context is
given what a context created under it prepares (Prepared.prepare_for on such a context, then set_matrix_prepared) -- the
upload that blz_set_matrix makes there.

The two expressions of the trace test are taken from the tool's source by name (the tool itself imports torch and bench.py
and opens its output file's directory: it is read, not imported).
"""
import ast
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import blz
import device_matrix_ref as dm
import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "device_matrix_cost.py")
DEV = "cuda:0"
P61, P16 = (1 << 61) - 1, 65521         # (65521: the largest prime below 2^16)
NAMES = ("rand300x200", "quirks40x30", "graph200x600")
_M = {}


def matrix(name, p):
    if (name, p) not in _M:
        _M[(name, p)] = (blz.Matrix.load(dm.path(name), p), orc.Matrix.load(dm.path(name), p))
    return _M[(name, p)]


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def triplets(M, ones):
    ti = torch.from_numpy(M.i).to(DEV)
    tj = torch.from_numpy(M.j).to(DEV)
    tx = None if ones else torch.from_numpy(M.x.view(np.int32)).to(DEV)
    return ti, tj, tx


# ---- the installs.  Each sets M on ctx as a left or right kernel and returns the high limbs it gave the entries, if any

def host(ctx, M, right):
    ctx.set_matrix(M, right)


def host_no_reorder(ctx, M, right):
    with env(BLZ_NO_REORDER="1"), blz.Context(ctx.prime, ctx.n) as plain:
        P = blz.Prepared.prepare_for(plain, M, right, 1)
    with P:
        ctx.set_matrix_prepared(P)


def high_limbs(ctx, M):
    hi = np.random.default_rng(M.nnz).integers(0, (ctx.prime >> 32) - 1, M.nnz).astype(np.uint32)
    hi[0] = 1
    return hi


def host_wide(ctx, M, right):
    hi = high_limbs(ctx, M)
    ctx.set_matrix(blz.Matrix(M.nrows, M.ncols, M.i, M.j, M.x, x_hi=hi), right)
    return hi


def device(ctx, M, right, reorder=False, ones=False):
    ti, tj, tx = triplets(M, ones)
    ctx.set_matrix_device(ti, tj, tx, nrows=M.nrows, ncols=M.ncols, right=right, reorder=reorder)


def device_wide(ctx, M, right):
    hi = high_limbs(ctx, M)
    ti, tj, _ = triplets(M, True)
    tx = torch.from_numpy(((hi.astype(np.uint64) << np.uint64(32)) | M.x).view(np.int64)).to(DEV)
    ctx.set_matrix_device(ti, tj, tx, nrows=M.nrows, ncols=M.ncols, right=right)
    return hi


def upload_ordered(ctx, M, right):
    ctx.set_matrix_upload(M, right, reorder=True)


# (the step, the call, its arguments, what it leaves behind: matrix_device_built, matrix_device_order, values_wide and
# whether a numbering is resident -- None: the host's scored choice decides, the fresh context says which)
HOST_WIDE = ("host, wide", host_wide, {}, (False, 0, True, None))
STEPS = (
    ("host, renumbered", host, {}, (False, 0, False, None)),
    ("device, ordered", device, dict(reorder=True), (True, 1, False, True)),
    ("host, BLZ_NO_REORDER=1", host_no_reorder, {}, (False, 0, False, False)),
    ("device, plain", device, {}, (True, 0, False, False)),
    ("device, wide", device_wide, {}, (True, 0, True, False)),
    ("device, plain, ones", device, dict(ones=True), (True, 0, False, False)),
    ("upload, ordered", upload_ordered, {}, (True, 1, False, True)),
    ("host, renumbered", host, {}, (False, 0, False, None)),
)


def steps_of(ctx):
    if ctx.word_bytes == 8:
        return (HOST_WIDE,) + STEPS
    return tuple(s for s in STEPS if s[1] is not device_wide)


def state(ctx):
    out = {}
    for t in (False, True):
        out["plan", t] = ctx.plan(t, 0)
        out["local_nnz", t] = ctx.local_nnz(t)
        out["matrix_stream_bytes", t] = ctx.matrix_stream_bytes(t)
        out["slab_wide", t] = ctx.slab_wide(t)
        out["slab_signed", t] = ctx.slab_signed(t)
        out["panel_rows", t] = ctx.panel_rows(t)
    out["locality"] = ctx.locality()
    for b in (blz.V, blz.TMP):
        out["rows", b] = ctx.rows(b)
        out["local_rows", b] = ctx.local_rows(b)
        has, perm = ctx.numbering(b)
        out["numbering", b] = (has, perm.tobytes())
    out["device_built"] = ctx.matrix_device_built()
    out["device_order"] = ctx.matrix_device_order()
    out["values_wide"] = ctx.values_wide()
    return out


def oracle_product(Mo, hi, ones, Xw, transpose, n, p):
    """M X mod p from the oracle's product of the low limbs (and, wide, of the high ones: M = M_lo + 2^32 M_hi)"""
    parts = Mo
    if ones:
        parts = orc.Matrix(Mo.nrows, Mo.ncols, Mo.i, Mo.j, np.ones(Mo.nnz, dtype=np.uint32))
    y = orc.spmv(parts, Xw.reshape(-1), transpose, n, p)
    if hi is not None:
        yh = orc.spmv(orc.Matrix(Mo.nrows, Mo.ncols, Mo.i, Mo.j, hi), Xw.reshape(-1), transpose, n, p)
        y = ((y.astype(object) + (1 << 32) * yh.astype(object)) % p).astype(np.uint64)
    return y


def apply_words(ctx, transpose, Xw, n):
    x = torch.from_numpy(np.ascontiguousarray(Xw, dtype=np.uint64).reshape(-1, n).view(np.int64)).to(DEV)
    y = ctx.apply(transpose, x)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint64).reshape(-1)


@pytest.mark.parametrize("p, n", ((P61, 8), (P16, 4)))
def test_an_install_leaves_no_trace_of_the_matrix_before_it(p, n):
    with blz.Context(p, n) as ctx:
        for k, (what, call, kw, leaves) in enumerate(steps_of(ctx)):
            M, Mo = matrix(NAMES[k % 3], p)
            right = bool(k % 2)
            hi = call(ctx, M, right, **kw)
            with blz.Context(p, n) as fresh:
                call(fresh, M, right, **kw)
                got, want = state(ctx), state(fresh)
            for key in want:
                assert got[key] == want[key], (k, what, key, got[key], want[key])
            assert (got["device_built"], got["device_order"], got["values_wide"]) == leaves[:3], (k, what)
            if leaves[3] is not None:
                assert got["numbering", blz.V][0] == got["numbering", blz.TMP][0] == leaves[3], (k, what)
            assert got["slab_wide", False] == got["slab_wide", True] == (hi is not None), (k, what)
            for transpose in (False, True):
                Xw = dm.residues(M.nrows if transpose else M.ncols, n, p, 5 + k)
                want_y = oracle_product(Mo, hi, kw.get("ones", False), Xw, transpose, n, p)
                assert np.array_equal(apply_words(ctx, transpose, Xw, n), want_y), (k, what, "transpose", transpose)


# ---- the trace lines

def tool_expressions():
    """TRACE and ORDER_TRACE of tools/device_matrix_cost.py, from its source"""
    found = {}
    with open(TOOL) as f:
        for node in ast.parse(f.read()).body:
            if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("TRACE", "ORDER_TRACE"):
                found[node.targets[0].id] = re.compile(ast.literal_eval(node.value.args[0]))
    return found["TRACE"], found["ORDER_TRACE"]


TRACE_SCRIPT = """
import os, sys
import blz
p, n = (1 << 61) - 1, 8
M = blz.Matrix.load(sys.argv[1], p)
for mark, trace, order in (("none-0", None, False), ("none-1", None, True), ("order-0", "1", False), ("order-1", "1", True)):
    sys.stderr.write("== %s\\n" % mark)
    sys.stderr.flush()
    os.environ.pop("BLZ_DEVMAT_TRACE", None)
    if trace:
        os.environ["BLZ_DEVMAT_TRACE"] = trace
    with blz.Context(p, n) as ctx:
        ctx.set_matrix_upload(M, False, reorder=order)
        assert ctx.matrix_device_built() and ctx.matrix_device_order() == int(order)
"""


def test_the_trace_lines_are_those_the_cost_tool_parses():
    TRACE, ORDER_TRACE = tool_expressions()
    path = os.pathsep.join(p for p in sys.path if p)
    run = subprocess.run([sys.executable, "-c", TRACE_SCRIPT, dm.path("rand300x200")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, PYTHONPATH=path))
    assert run.returncode == 0, run.stderr
    phase = {}
    for line in run.stderr.splitlines():
        if line.startswith("== "):
            cur = phase.setdefault(line[3:], [])
        elif TRACE.search(line) or ORDER_TRACE.search(line) or line.startswith("blz device"):
            cur.append(line)
    assert sorted(phase) == ["none-0", "none-1", "order-0", "order-1"]
    assert phase["none-0"] == [] and phase["none-1"] == []
    assert len(phase["order-0"]) == 1 and TRACE.search(phase["order-0"][0]) and not ORDER_TRACE.search(phase["order-0"][0])
    assert len(phase["order-1"]) == 2
    first, second = phase["order-1"]
    assert ORDER_TRACE.search(first) and not TRACE.search(first)
    assert TRACE.search(second) and not ORDER_TRACE.search(second)
    lines = run.stderr.splitlines()
    assert lines.index(second) == lines.index(first) + 1       # directly in front of it
