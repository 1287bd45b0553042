#!/usr/bin/env python3
"""What the 32-bit device-block calls cost beside their 64-bit namesakes on the same residues, widened.

Blocks of the GL7d19 row count (1 911 130 rows), p = 2^31 - 1 and 2^32 - 5, n = 1, 8, 16 and 64.  Cells: dot; dot_pair(v, Av, Av);
combine with 2 and 3 terms; combine_pair in place (the update of a Lanczos step); and, on the GL7d19-shape synthetic of
bench.py at p = 2^31 - 1: set + get of a block, and apply.

Method: HIP events on the caller's stream around a region of 20 calls back to back; the two families alternated A B A B, five
regions each, in one process on one GPU; a figure is the median region, and every cell carries its min-max spread.  Before a
cell is timed its two results are compared word for word.  A difference counts only where it exceeds the larger spread of the
two cells.  Bytes are the blocks a call must read and write once (rows x n x word size each), over the median time.

Recorded, not gated.  There is no CPU path: without a GPU this fails.

Usage: tools/device_w32_cost.py [--out profiles/device_w32_cost.txt] [--rows N] [--skip-matrix]
One process, one GPU step: run it under a time limit of its own (`timeout -k 10 540 python tools/device_w32_cost.py`; the
whole table takes under a minute) and chain whatever follows with `&&`.  The table is written line by line as it is measured.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))
sys.path.insert(0, ROOT)
import blz  # noqa: E402
from bench import WORKLOADS  # noqa: E402

P31, P32 = (1 << 31) - 1, (1 << 32) - 5
REGIONS, CALLS = 5, 20
DEV = "cuda:0"
OUT = None                                              # the file the table goes to, line by line


def say(line=""):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def region(fn):
    """device time of one fn() in us: HIP events on torch's current stream around CALLS calls back to back"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / CALLS


def alternated(f32, f64):
    for fn in (f32, f64, f32, f64):                     # code objects, scratch, events: before the clock
        fn()
    torch.cuda.synchronize()
    t32, t64 = [], []
    for _ in range(REGIONS):                            # A B A B
        t32.append(region(f32))
        t64.append(region(f64))
    return t32, t64


def cell(what, t32, t64, bytes32, bytes64):
    m32, m64 = statistics.median(t32), statistics.median(t64)
    s32, s64 = max(t32) - min(t32), max(t64) - min(t64)
    spread = max(s32, s64)
    if abs(m64 - m32) <= spread:
        verdict = "no difference beyond the spread"
    elif m32 < m64:
        verdict = "32-bit faster: %.2fx" % (m64 / m32)
    else:
        verdict = "32-bit SLOWER: %.2fx" % (m64 / m32)
    say("   %-34s u32 %9.1f us (%9.1f .. %9.1f) %6.2f TB/s;  u64 %9.1f us (%9.1f .. %9.1f) %6.2f TB/s;  %s"
        % (what, m32, min(t32), max(t32), bytes32 / m32 * 1e-6, m64, min(t64), max(t64), bytes64 / m64 * 1e-6, verdict))


def block32(rows, n, p, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, p, (rows, n), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)


def widen(t):
    return t.to(torch.int64) & 0xFFFFFFFF


def same(z32, z64):
    return torch.equal(widen(z32), z64.view(torch.int64))


def section_algebra(rows):
    for p, pname in ((P31, "2^31 - 1"), (P32, "2^32 - 5")):
        say("p = %s, %d rows; us per call, median of %d regions of %d calls (min .. max), A B A B" % (pname, rows, REGIONS, CALLS))
        for n in (1, 8, 16, 64):
            v, Av, pb = (block32(rows, n, p, 3 * n + k) for k in range(3))
            V, AV, PB = widen(v), widen(Av), widen(pb)
            g = torch.Generator(device=DEV)
            g.manual_seed(99)
            coef = torch.randint(0, p, (5, n, n), dtype=torch.int64, device=DEV, generator=g)
            c1, c1w, c2, c2w = (torch.empty(s, dtype=torch.uint64, device=DEV) for s in ((n, n), (n, n), (2, n, n), (2, n, n)))
            z, Z = torch.empty_like(v), torch.empty_like(V)
            blk = rows * n
            with blz.Context(p, n) as ctx:
                assert ctx.word_bytes == 4
                ctx.dot32(v, Av, out=c1), ctx.dot(V, AV, out=c1w)
                assert torch.equal(c1.view(torch.int64), c1w.view(torch.int64))
                cell("n = %2d  dot(v, Av)" % n, *alternated(lambda: ctx.dot32(v, Av, out=c1), lambda: ctx.dot(V, AV, out=c1w)),
                     2 * blk * 4, 2 * blk * 8)
                ctx.dot_pair32(v, Av, Av, out=c2), ctx.dot_pair(V, AV, AV, out=c2w)
                assert torch.equal(c2.view(torch.int64), c2w.view(torch.int64))
                cell("n = %2d  dot_pair(v, Av, Av)" % n, *alternated(lambda: ctx.dot_pair32(v, Av, Av, out=c2),
                                                                     lambda: ctx.dot_pair(V, AV, AV, out=c2w)), 2 * blk * 4, 2 * blk * 8)
                for nterms in (2, 3):
                    t32 = [(x, coef[k]) for k, x in enumerate((Av, v, pb)[:nterms])]
                    t64 = [(x, coef[k]) for k, x in enumerate((AV, V, PB)[:nterms])]
                    ctx.combine32(t32, out=z), ctx.combine(t64, out=Z)
                    assert same(z, Z)
                    cell("n = %2d  combine, %d terms" % (n, nterms), *alternated(lambda: ctx.combine32(t32, out=z),
                                                                                lambda: ctx.combine(t64, out=Z)),
                         (nterms + 1) * blk * 4, (nterms + 1) * blk * 8)
                # the update of a step, in place on v and p: the words change from call to call, the work does not
                u32 = [(Av, coef[0], None), (v, coef[1], coef[4]), (pb, coef[2], coef[3])]
                u64 = [(AV, coef[0], None), (V, coef[1], coef[4]), (PB, coef[2], coef[3])]
                ctx.combine_pair32(u32, out=(v, pb)), ctx.combine_pair(u64, out=(V, PB))
                assert same(v, V) and same(pb, PB)
                cell("n = %2d  combine_pair, in place" % n, *alternated(lambda: ctx.combine_pair32(u32, out=(v, pb)),
                                                                       lambda: ctx.combine_pair(u64, out=(V, PB))),
                     5 * blk * 4, 5 * blk * 8)
            del v, Av, pb, V, AV, PB, z, Z
            torch.cuda.empty_cache()
        say()


def section_matrix():
    w = WORKLOADS["gl7d19"]
    p, n, right = P31, w["n"], w["right"]
    say("the GL7d19-shape synthetic of bench.py (%d x %d, %d entries), n = %d, p = 2^31 - 1" % (w["rows"], w["cols"], w["nnz"], n))
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=w["pattern"])
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M, right)
        xr, yr = ctx.apply_rows(not right)
        x = block32(xr, n, p, 7)
        X = widen(x)
        y, Y = torch.empty((yr, n), dtype=torch.int32, device=DEV), torch.empty((yr, n), dtype=torch.int64, device=DEV)
        back, BACK = torch.empty_like(x), torch.empty_like(X)
        assert ctx.rows(blz.V) == xr

        def io32():
            ctx.set_block_device32(blz.V, x)
            ctx.get_block_device32(blz.V, out=back)

        def io64():
            ctx.set_block_device(blz.V, X)
            ctx.get_block_device(blz.V, out=BACK)
        io32(), io64()
        assert torch.equal(back, x) and torch.equal(BACK, X)
        cell("n = %2d  set + get" % n, *alternated(io32, io64), 4 * xr * n * 4, 2 * xr * n * (4 + 8))
        ctx.apply32(not right, x, out=y), ctx.apply(not right, X, out=Y)
        assert same(y, Y)
        cell("n = %2d  apply" % n, *alternated(lambda: ctx.apply32(not right, x, out=y), lambda: ctx.apply(not right, X, out=Y)),
             (xr + yr) * n * 4, (xr + yr) * n * 8)
    say("   (bytes of set + get: the caller's block and the 4-byte slab, each once per direction; of apply: the caller's two blocks")
    say("    only -- the product's own traffic is the same on both sides)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_w32_cost.txt"))
    ap.add_argument("--rows", type=int, default=WORKLOADS["gl7d19"]["rows"])
    ap.add_argument("--skip-matrix", action="store_true", help="leave out set + get and apply (the full-size matrix)")
    args = ap.parse_args()
    if blz.device_count() < 1:
        raise SystemExit("device_w32_cost: no GPU visible -- nothing here runs on a CPU")
    global OUT
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")
    say("32-bit device blocks beside their 64-bit namesakes on the same residues (tools/device_w32_cost.py), %s"
        % torch.cuda.get_device_name(0))
    say("a difference counts only where it exceeds the larger min-max spread of the two cells")
    say()
    section_algebra(args.rows)
    if not args.skip_matrix:
        section_matrix()
    OUT.close()


if __name__ == "__main__":
    main()
