"""The two word widths of the device-block family refuse alike: every faulty call below goes through a 64-bit call and its
...32 namesake, by raw ctypes, on ONE context that serves both families (p = 2^31 - 1, n = 8, a 64 x 48 matrix, blocks of 64
rows).  Both must return BLZ_EINVAL, and the two messages must be the same text once the 32-bit one is read in 64-bit terms:
the "32" at the end of the function's name dropped, "4 bytes" read as "8 bytes", and the two byte counts of an overrun ("needs
N bytes ... its allocation ends after M", which count 4-byte words on one side and 8-byte words on the other: the same rows, the
same stride, half the bytes) doubled.  No fault of the table launches a kernel: every output holds its sentinel at the end.

The entry refusals that belong to the 32-bit family alone (device blocks on ranks switched on, a communicator, a context whose
word is not 4 bytes) are not in the table; tests/test_gpu_device_w32.py has them.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import blz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, N, ROWS, COLS, NNZ, SEED = (1 << 31) - 1, 8, 64, 48, 300, 0x50415249
SENT = 0x5A


def vp(x):
    return C.c_void_p(x)


class Family:
    """the eight calls of one word width on buffers of that width: blocks of ROWS rows, every word four SENT bytes"""

    def __init__(self, ctx, word, hip):
        self.ctx, self.word, self.sfx, self.hip = ctx, word, "" if word == 8 else "32", hip
        dtype = torch.int64 if word == 8 else torch.int32
        fill = int.from_bytes(bytes([SENT]) * 4, "little")     # a residue below P at either width
        self.tensors = [torch.full((ROWS, N), fill, dtype=dtype, device=DEV) for _ in range(4)]
        self.tensors.append(torch.full((2 * ROWS, N), fill, dtype=dtype, device=DEV))
        self.X, self.Y, self.Z, self.W, self.B = (t.data_ptr() for t in self.tensors)
        short = C.c_void_p()                            # an allocation of exactly ROWS - 1 rows (torch's come out of larger ones)
        assert hip.hipMalloc(C.byref(short), C.c_size_t((ROWS - 1) * N * word)) == 0
        self.S = short.value
        self.row = N * word                             # bytes of a row at stride n
        self.block = blz.V if ctx.rows(blz.V) == ROWS else blz.TMP     # the block of ROWS rows

    def close(self):
        assert self.hip.hipFree(vp(self.S)) == 0

    def fn(self, name):
        return getattr(blz.lib(), f"blz_{name}_device{self.sfx}")

    def set(self, x, ld, stream=None, block=None):
        return self.fn("set_block")(self.ctx.h, C.c_int(self.block if block is None else block), vp(x), C.c_int64(ld), stream, None)

    def get(self, x, ld, stream=None, block=None):
        return self.fn("get_block")(self.ctx.h, C.c_int(self.block if block is None else block), vp(x), C.c_int64(ld), stream)

    def apply(self, x, ldx, y, ldy, stream=None):       # y = M x: x has COLS rows, y has ROWS
        return self.fn("apply")(self.ctx.h, C.c_int(0), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), stream)

    def apply2(self, x, ldx, y, ldy, z, ldz, stream=None):     # z = M^T (M x): x and z have COLS rows, y has ROWS
        return self.fn("apply_pair")(self.ctx.h, C.c_int(0), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), vp(z), C.c_int64(ldz),
                                     stream)

    def dot(self, rows, x, ldx, y, ldy, c, stream=None):
        return self.fn("dot")(self.ctx.h, C.c_int64(rows), vp(x), C.c_int64(ldx), vp(y), C.c_int64(ldy), vp(c), stream)

    def dot2(self, rows, x0, ld0, x1, ld1, y, ldy, c, stream=None):
        return self.fn("dot_pair")(self.ctx.h, C.c_int64(rows), vp(x0), C.c_int64(ld0), vp(x1), C.c_int64(ld1), vp(y),
                                   C.c_int64(ldy), vp(c), stream)

    def combine(self, rows, xs, lds, a, z, ldz, stream=None, nterms=None):
        k = len(xs)
        return self.fn("combine")(self.ctx.h, C.c_int64(rows), C.c_int(k if nterms is None else nterms), (C.c_void_p * k)(*xs),
                                  (C.c_int64 * k)(*lds), (C.c_void_p * k)(*a), vp(z), C.c_int64(ldz), stream)

    def combine2(self, rows, xs, lds, a0, a1, z0, ldz0, z1, ldz1, stream=None, nterms=None):
        k = len(xs)
        return self.fn("combine_pair")(self.ctx.h, C.c_int64(rows), C.c_int(k if nterms is None else nterms),
                                       (C.c_void_p * k)(*xs), (C.c_int64 * k)(*lds), (C.c_void_p * k)(*a0), (C.c_void_p * k)(*a1),
                                       vp(z0), C.c_int64(ldz0), vp(z1), C.c_int64(ldz1), stream)


def all_eight(f, A, Cc, stream=None):
    """the eight calls, well formed but for the stream"""
    n = N
    return (lambda: f.set(f.X, n, stream), lambda: f.get(f.Z, n, stream), lambda: f.apply(f.X, n, f.Z, n, stream),
            lambda: f.apply2(f.X, n, f.Z, n, f.W, n, stream), lambda: f.dot(ROWS, f.X, n, f.Y, n, Cc, stream),
            lambda: f.dot2(ROWS, f.X, n, f.Y, n, f.Y, n, Cc, stream),
            lambda: f.combine(ROWS, [f.X, f.Y], [n, n], [A, A], f.Z, n, stream),
            lambda: f.combine2(ROWS, [f.X, f.Y], [n, n], [A, A], [A, A], f.Z, n, f.W, n, stream))


def faults(A, Cc, H, HS):
    """(what the message must name, the faulty call as a function of the family).  A: an n x n coefficient, Cc: 2 n^2 words for
    a result (both u64 on the device in either family), H / HS: host memory."""
    n, r = N, ROWS
    last = COLS - 1                                     # the last row of a block of COLS rows
    five = lambda v: [v] * 5
    return [
        # a NULL block
        ("dev is NULL", lambda f: f.set(0, n)), ("dev is NULL", lambda f: f.get(0, n)),
        ("x is NULL", lambda f: f.apply(0, n, f.Z, n)), ("y is NULL", lambda f: f.apply(f.X, n, 0, n)),
        ("x is NULL", lambda f: f.apply2(0, n, f.Z, n, f.W, n)), ("z is NULL", lambda f: f.apply2(f.X, n, f.Z, n, 0, n)),
        ("x is NULL", lambda f: f.dot(r, 0, n, f.Y, n, Cc)), ("y is NULL", lambda f: f.dot(r, f.X, n, 0, n, Cc)),
        ("c is NULL", lambda f: f.dot(r, f.X, n, f.Y, n, 0)), ("x1 is NULL", lambda f: f.dot2(r, f.X, n, 0, n, f.Y, n, Cc)),
        ("c is NULL", lambda f: f.dot2(r, f.X, n, f.Y, n, f.Y, n, 0)),
        ("x[0] is NULL", lambda f: f.combine(r, [0], [n], [A], f.Z, n)), ("a[0] is NULL", lambda f: f.combine(r, [f.X], [n], [0], f.Z, n)),
        ("z is NULL", lambda f: f.combine(r, [f.X], [n], [A], 0, n)),
        ("x[1] is NULL", lambda f: f.combine2(r, [f.X, 0], [n, n], [A, A], [A, A], f.Z, n, f.W, n)),
        ("z1 is NULL", lambda f: f.combine2(r, [f.X], [n], [A], [A], f.Z, n, 0, n)),
        # a host pointer
        (" dev = ", lambda f: f.set(H, n)), (" dev = ", lambda f: f.get(H, n)),
        (" x = ", lambda f: f.apply(H, n, f.Z, n)), (" y = ", lambda f: f.apply2(f.X, n, H, n, f.Z, n)),
        (" x = ", lambda f: f.dot(r, H, n, f.Y, n, Cc)), (" c = ", lambda f: f.dot(r, f.X, n, f.Y, n, HS)),
        (" x1 = ", lambda f: f.dot2(r, f.X, n, H, n, f.Y, n, Cc)), (" c = ", lambda f: f.dot2(r, f.X, n, f.Y, n, f.Y, n, HS)),
        (" z = ", lambda f: f.combine(r, [f.X], [n], [A], H, n)), (" a[0] = ", lambda f: f.combine(r, [f.X], [n], [HS], f.Z, n)),
        (" x[1] = ", lambda f: f.combine2(r, [f.X, H], [n, n], [A, A], [A, A], f.Z, n, f.W, n)),
        (" a1[0] = ", lambda f: f.combine2(r, [f.X], [n], [A], [HS], f.Z, n, f.W, n)),
        # a stride of n - 1
        ("stride of dev", lambda f: f.set(f.X, n - 1)), ("stride of dev", lambda f: f.get(f.Z, n - 1)),
        ("stride of y", lambda f: f.apply(f.X, n, f.Z, n - 1)), ("stride of x", lambda f: f.apply2(f.X, n - 1, 0, 0, f.Z, n)),
        ("stride of x", lambda f: f.dot(r, f.X, n - 1, f.Y, n, Cc)), ("stride of y", lambda f: f.dot2(r, f.X, n, f.Y, n, f.Y, n - 1, Cc)),
        ("stride of x[1]", lambda f: f.combine(r, [f.X, f.Y], [n, n - 1], [A, A], f.Z, n)),
        ("stride of z0", lambda f: f.combine2(r, [f.X], [n], [A], [A], f.Z, n - 1, f.W, n)),
        # half a word off the word's alignment (and the 8-byte operands, four bytes off in either family)
        ("dev is not aligned", lambda f: f.set(f.B + f.word // 2, n)), ("dev is not aligned", lambda f: f.get(f.B + f.word // 2, n)),
        ("y is not aligned", lambda f: f.apply(f.X, n, f.B + f.word // 2, n)),
        ("z is not aligned", lambda f: f.apply2(f.X, n, 0, 0, f.B + f.word // 2, n)),
        ("x is not aligned", lambda f: f.dot(r - 1, f.X + f.word // 2, n, f.Y, n, Cc)),
        ("y is not aligned", lambda f: f.dot(r - 1, f.X, n, f.Y + f.word // 2, n, Cc)),
        ("x0 is not aligned", lambda f: f.dot2(r - 1, f.X + f.word // 2, n, f.Y, n, f.Y, n, Cc)),
        ("z is not aligned", lambda f: f.combine(r - 1, [f.X], [n], [A], f.Z + f.word // 2, n)),
        ("z1 is not aligned", lambda f: f.combine2(r - 1, [f.X], [n], [A], [A], f.Z, n, f.W + f.word // 2, n)),
        ("c is not aligned to 8", lambda f: f.dot(r, f.X, n, f.Y, n, Cc + 4)),
        ("a[0] is not aligned to 8", lambda f: f.combine(r, [f.X], [n], [A + 4], f.Z, n)),
        # one row past the allocation
        ("dev needs", lambda f: f.set(f.S, n)), ("dev needs", lambda f: f.get(f.S, n)),
        ("y needs", lambda f: f.apply(f.X, n, f.S, n)), ("y needs", lambda f: f.apply2(f.X, n, f.S, n, f.Z, n)),
        ("x needs", lambda f: f.dot(r, f.S, n, f.Y, n, Cc)), ("y needs", lambda f: f.dot2(r, f.X, n, f.Y, n, f.S, n, Cc)),
        ("z needs", lambda f: f.combine(r, [f.X], [n], [A], f.S, n)),
        ("x[0] needs", lambda f: f.combine2(r, [f.S], [n], [A], [A], f.Z, n, f.W, n)),
        # every overlap form
        ("x and y overlap", lambda f: f.apply(f.B, n, f.B + last * f.row, n)),
        ("z overlaps x without", lambda f: f.apply2(f.B, n, 0, 0, f.B + f.row, n)),
        ("z overlaps x without", lambda f: f.apply2(f.B, n, 0, 0, f.B, n + 1)),
        ("y overlaps x", lambda f: f.apply2(f.B, n, f.B + last * f.row, n, f.W, n)),
        ("y overlaps z", lambda f: f.apply2(f.X, n, f.B + last * f.row, n, f.B, n)),
        ("c overlaps x", lambda f: f.dot(n, Cc, n, f.Y, n, Cc)), ("c overlaps y", lambda f: f.dot(n, f.X, n, Cc, n, Cc)),
        ("c overlaps x0", lambda f: f.dot2(n, Cc, n, f.X, n, f.Y, n, Cc)), ("c overlaps x1", lambda f: f.dot2(n, f.X, n, Cc, n, f.Y, n, Cc)),
        ("c overlaps y", lambda f: f.dot2(n, f.X, n, f.Y, n, Cc, n, Cc)),
        ("z overlaps x[0] without", lambda f: f.combine(r, [f.B, f.Y], [n, n], [A, A], f.B + f.row, n)),
        ("z overlaps x[0] without", lambda f: f.combine(r // 2, [f.B, f.Y], [n, n], [A, A], f.B, 2 * n)),
        ("z overlaps a[0]", lambda f: f.combine(n, [f.X], [n], [f.B], f.B, n)),
        ("z0 overlaps z1", lambda f: f.combine2(r, [f.X, f.Y], [n, n], [A, A], [A, A], f.B, n, f.B + (r - 1) * f.row, n)),
        ("z0 overlaps z1", lambda f: f.combine2(r, [f.X, f.Y], [n, n], [A, A], [A, A], f.X, n, f.X, n)),
        ("z1 overlaps x[1] without", lambda f: f.combine2(r // 2, [f.X, f.B], [n, n], [A, A], [A, A], f.Z, n, f.B, 2 * n)),
        ("z0 overlaps a1[0]", lambda f: f.combine2(n, [f.X], [n], [A], [f.B], f.B, n, f.W, n)),
        # nterms of 0 and of 5
        ("nterms = 0", lambda f: f.combine(r, [], [], [], f.Z, n)), ("nterms = 5", lambda f: f.combine(r, five(f.X), five(n), five(A), f.Z, n)),
        ("nterms = 0", lambda f: f.combine2(r, [], [], [], [], f.Z, n, f.W, n)),
        ("nterms = 5", lambda f: f.combine2(r, five(f.X), five(n), five(A), five(A), f.Z, n, f.W, n)),
        # rows = -1
        ("rows = -1", lambda f: f.dot(-1, f.X, n, f.Y, n, Cc)), ("rows = -1", lambda f: f.dot2(-1, f.X, n, f.Y, n, f.Y, n, Cc)),
        ("rows = -1", lambda f: f.combine(-1, [f.X], [n], [A], f.Z, n)),
        ("rows = -1", lambda f: f.combine2(-1, [f.X], [n], [A], [A], f.Z, n, f.W, n)),
        # a term in neither output, an output with no term
        ("term 1 enters neither", lambda f: f.combine2(r, [f.X, f.Y], [n, n], [A, 0], [A, 0], f.Z, n, f.W, n)),
        ("z1 has no term", lambda f: f.combine2(r, [f.X, f.Y], [n, n], [A, A], [0, 0], f.Z, n, f.W, n)),
        ("z0 has no term", lambda f: f.combine2(r, [f.X], [n], [0], [A], f.Z, n, f.W, n)),
        # an unknown block index
        ("block 7", lambda f: f.set(f.X, n, block=7)), ("block -1", lambda f: f.get(f.Z, n, block=-1)),
    ]


def as64(msg):
    """a message of the 32-bit family read in 64-bit terms"""
    msg = re.sub(r"\b(blz_\w+_device)32\b", r"\1", msg)
    msg = re.sub(r"(needs |ends after )(\d+)", lambda m: m.group(1) + str(2 * int(m.group(2))), msg)
    return re.sub(r"\b4 bytes", "8 bytes", msg)


def last_error():
    return blz.lib().blz_last_error().decode()


def test_both_widths_refuse_alike():
    hip = C.CDLL("libamdhip64.so.7")                    # the runtime the process already uses
    M = blz.Matrix.synth(ROWS, COLS, NNZ, SEED, P)
    coef = torch.full((N, N), 3, dtype=torch.int64, device=DEV)
    res = torch.full((2, N, N), int.from_bytes(bytes([SENT]) * 8, "little"), dtype=torch.int64, device=DEV)
    A, Cc = coef.data_ptr(), res.data_ptr()
    hb, hs = np.zeros((ROWS, N), dtype=np.uint64), np.zeros((2, N, N), dtype=np.uint64)
    with blz.Context(P, N) as ctx:
        ctx.set_matrix(M)
        assert ctx.word_bytes == 4 and ctx.apply_rows(False) == (COLS, ROWS)
        wide, narrow = Family(ctx, 8, hip), Family(ctx, 4, hip)
        try:
            for f in (wide, narrow):                    # the calls the table spoils are well formed
                for call in all_eight(f, A, Cc):
                    assert call() == blz.OK, last_error()
            torch.cuda.synchronize()
            snapshot = [[t.clone() for t in f.tensors] for f in (wide, narrow)]
            kept = res.clone()
            got = []
            for part, call in faults(A, Cc, hb.ctypes.data, hs.ctypes.data):
                pair = []
                for f in (wide, narrow):
                    rc = call(f)
                    pair.append((rc, last_error()))
                got.append((part, pair))
            # a stream that is capturing (captured and thrown away: never replayed)
            s = torch.cuda.Stream(device=DEV)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for c8, c4 in zip(all_eight(wide, A, Cc, h), all_eight(narrow, A, Cc, h)):
                    pair = []
                    for call in (c8, c4):
                        rc = call()
                        pair.append((rc, last_error()))
                    got.append(("capturing", pair))
                coef.add_(0)                            # (a graph of one node, not an empty one)
            for part, ((rc8, m8), (rc4, m4)) in got:
                assert rc8 == blz.EINVAL and rc4 == blz.EINVAL, (part, rc8, m8, rc4, m4)
                assert part in m8, (part, m8)
                assert as64(m4) == m8, (m8, m4)
                assert "device32" in m4 or "no matrix" in m4, m4
            # nothing ran: every buffer is what it was after the well-formed calls
            torch.cuda.synchronize()
            for f, was in zip((wide, narrow), snapshot):
                for t, w in zip(f.tensors, was):
                    assert torch.equal(t, w)
            assert torch.equal(res, kept)
        finally:
            torch.cuda.synchronize()
            wide.close()
            narrow.close()
