#!/usr/bin/env python3
"""What setting the matrix costs, on the host and on the device.

Shapes: the GL7d19, relat9 and relat8 shapes of bench.py, triplets from Matrix.synth.  Per shape, wall time of
  (a) set_matrix as it stands (renumbering, CSR(M), CSR(M^T) on the host, upload);
  (b) set_matrix under BLZ_NO_REORDER=1 (the same host build without the renumbering);
  (c) set_matrix_device from triplets already resident on the GPU;
  (d) set_matrix_upload (host triplets copied to the device, then the build of (c));
alternated a b c d, ROUNDS rounds, each on a fresh context; a figure is the median round with its min .. max.  The kernels of
(c) are timed by HIP events inside the library (BLZ_DEVMAT_TRACE=1, one line on stderr per build, medians here).  After the
last round of (a), (b) and (c) the context iterates: ms per step of `iterate`, median of REGIONS regions of STEPS steps.
(b) and (c) run the same layout; (a) against (c) is the price of keeping the caller's numbering, stated next to the set-up
time saved and the iteration count at which the two cross.

With --order the legs are instead
  (a)  set_matrix as it stands;
  (a') set_matrix under BLZ_REORDER_PLAIN=1 BLZ_NO_PANEL=1 (blz_reorder's order, no scored choice, no hot rows, no panel);
  (c)  set_matrix_device from resident triplets, the caller's numbering kept;
  (e)  set_matrix_device(reorder=True): the same order as (a') made on the GPU, then the build of (c);
the kernels of (e)'s renumbering are timed by the same trace, and every leg iterates after its last round.  (a') and (e) run
the same row pointers; (e) - (c) is the price of the order, stated with the iteration counts at which (e) overtakes (c) and
(a) would overtake (e).

Recorded, not gated.  There is no CPU path: without a GPU this fails.

Usage: tools/device_matrix_cost.py [--out profiles/device_matrix_cost.txt] [--rounds 5] [--shapes gl7d19,relat9,relat8]
       tools/device_matrix_cost.py --order [--out profiles/device_order_cost.txt] ...
One process, one GPU step: run it under a time limit of its own and chain whatever follows with `&&`.  The table is written
line by line as it is measured.
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))
sys.path.insert(0, ROOT)
import blz  # noqa: E402
from bench import WORKLOADS  # noqa: E402

DEV = "cuda:0"
REGIONS, STEPS = 5, 20
OUT = None
TRACE = re.compile(r"check\+count ([0-9.]+) ms, scan ([0-9.]+) ms, scatter ([0-9.]+) ms, palette ([0-9.]+) ms, pack ([0-9.]+) ms")
ORDER_TRACE = re.compile(r"row keys ([0-9.]+) ms, row sort ([0-9.]+) ms, column keys ([0-9.]+) ms, column sort ([0-9.]+) ms, "
                         r"relabel ([0-9.]+) ms")


def say(line=""):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


class Stderr:
    """the process's stderr into a file for the length of a `with` (the library's trace line is written by C code)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def context(p, n, no_reorder=False):
    old = os.environ.get("BLZ_NO_REORDER")
    if no_reorder:
        os.environ["BLZ_NO_REORDER"] = "1"
    try:
        return blz.Context(p, n)
    finally:
        if no_reorder:
            if old is None:
                del os.environ["BLZ_NO_REORDER"]
            else:
                os.environ["BLZ_NO_REORDER"] = old


class PlainOrder:
    """BLZ_REORDER_PLAIN=1 BLZ_NO_PANEL=1 for the length of a `with` (read when the context is made and when the matrix is set)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("BLZ_REORDER_PLAIN", "BLZ_NO_PANEL")}
        if self.on:
            os.environ.update(BLZ_REORDER_PLAIN="1", BLZ_NO_PANEL="1")

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ms_per_step(ctx):
    ctx.init_v()
    ctx.iterate(3)
    out = []
    for _ in range(REGIONS):
        done, stopped, ms = ctx.iterate(STEPS)
        if done:
            out.append(ms / done)
        if stopped:
            break
    return out


def fmt(ts, unit="s", scale=1.0):
    return "%9.3f %s (%9.3f .. %9.3f)" % (statistics.median(ts) * scale, unit, min(ts) * scale, max(ts) * scale)


def shape(name, rounds):
    w = WORKLOADS[name]
    p, n, right = w["prime"], w["n"], w["right"]
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, w["pattern"])
    say("%s: %d x %d, %d entries, n = %d, p = %d, %s kernel" % (w["desc"], M.nrows, M.ncols, M.nnz, n, p, "right" if right else "left"))
    ti = torch.from_numpy(M.i).to(DEV)
    tj = torch.from_numpy(M.j).to(DEV)
    tx = torch.from_numpy(M.x.view("int32")).to(DEV)
    torch.cuda.synchronize()
    wall = {k: [] for k in "abcd"}
    kern = []
    steps = {}
    for r in range(rounds):
        last = r == rounds - 1
        for k in "abcd":
            ctx = context(p, n, no_reorder=(k == "b"))
            with Stderr() as err:
                t0 = time.perf_counter()
                if k in "ab":
                    ctx.set_matrix(M, right)
                elif k == "c":
                    ctx.set_matrix_device(ti, tj, tx, nrows=M.nrows, ncols=M.ncols, right=right)
                else:
                    ctx.set_matrix_upload(M, right)
                ctx.sync()
                wall[k].append(time.perf_counter() - t0)
            m = TRACE.search(err.text)
            if k == "c" and m:
                kern.append([float(g) for g in m.groups()])
            if last and k in "abc":
                steps[k] = ms_per_step(ctx)
            ctx.close()
    say("   (a) set_matrix                         %s" % fmt(wall["a"]))
    say("   (b) set_matrix, BLZ_NO_REORDER=1       %s" % fmt(wall["b"]))
    say("   (c) set_matrix_device, resident        %s" % fmt(wall["c"]))
    say("   (d) set_matrix_upload                  %s" % fmt(wall["d"]))
    if kern:
        for q, what in enumerate(("check + count", "scan (2 x 3 launches)", "scatter", "palette", "pack (both slabs)")):
            col = [row[q] for row in kern]
            say("       kernel  %-24s %s" % (what, fmt(col, "ms")))
    for k, what in (("a", "after (a)"), ("b", "after (b)"), ("c", "after (c)")):
        if steps.get(k):
            say("   iterate %-10s                     %s per step" % (what, fmt(steps[k], "ms")))
    if steps.get("a") and steps.get("c") and steps.get("b"):
        sa, sb, sc = (statistics.median(steps[k]) for k in "abc")
        spread = max(max(steps[k]) - min(steps[k]) for k in "bc")
        say("   (b) against (c), same layout: %+.4f ms per step, larger spread of the two %.4f ms: %s"
            % (sc - sb, spread, "no difference beyond the spread" if abs(sc - sb) <= spread else "A DIFFERENCE TO EXPLAIN"))
        saved = statistics.median(wall["a"]) - statistics.median(wall["c"])
        price = sc - sa
        if price > 0:
            say("   keeping the caller's numbering costs %.4f ms per step and saves %.3f s of set-up: the two cross after %d iterations"
                % (price, saved, int(saved * 1e3 / price)))
        else:
            say("   keeping the caller's numbering costs nothing per step here (%+.4f ms) and saves %.3f s of set-up" % (price, saved))
    say()
    del ti, tj, tx


def shape_order(name, rounds):
    w = WORKLOADS[name]
    p, n, right = w["prime"], w["n"], w["right"]
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, w["pattern"])
    say("%s: %d x %d, %d entries, n = %d, p = %d, %s kernel" % (w["desc"], M.nrows, M.ncols, M.nnz, n, p, "right" if right else "left"))
    ti = torch.from_numpy(M.i).to(DEV)
    tj = torch.from_numpy(M.j).to(DEV)
    tx = torch.from_numpy(M.x.view("int32")).to(DEV)
    torch.cuda.synchronize()
    legs = ("a", "p", "c", "e")
    wall = {k: [] for k in legs}
    kern, build = [], []
    steps = {}
    for r in range(rounds):
        last = r == rounds - 1
        for k in legs:
            with PlainOrder(k == "p"):
                ctx = context(p, n)
                with Stderr() as err:
                    t0 = time.perf_counter()
                    if k in "ap":
                        ctx.set_matrix(M, right)
                    else:
                        ctx.set_matrix_device(ti, tj, tx, nrows=M.nrows, ncols=M.ncols, right=right, reorder=(k == "e"))
                    ctx.sync()
                    wall[k].append(time.perf_counter() - t0)
            if k == "e":
                m, b = ORDER_TRACE.search(err.text), TRACE.search(err.text)
                if m:
                    kern.append([float(g) for g in m.groups()])
                if b:
                    build.append(sum(float(g) for g in b.groups()))
            if last:
                steps[k] = ms_per_step(ctx)
            ctx.close()
    say("   (a)  set_matrix                                     %s" % fmt(wall["a"]))
    say("   (a') set_matrix, BLZ_REORDER_PLAIN=1 BLZ_NO_PANEL=1 %s" % fmt(wall["p"]))
    say("   (c)  set_matrix_device, numbering kept              %s" % fmt(wall["c"]))
    say("   (e)  set_matrix_device, reorder=True                %s" % fmt(wall["e"]))
    if kern:
        for q, what in enumerate(("row keys (fill + minimum)", "row sort", "column keys (fill + minimum)", "column sort", "relabel")):
            say("        kernel  %-30s %s" % (what, fmt([row[q] for row in kern], "ms")))
    if build:
        say("        kernel  %-30s %s" % ("the build's own five passes", fmt(build, "ms")))
    names = {"a": "after (a)", "p": "after (a')", "c": "after (c)", "e": "after (e)"}
    for k in legs:
        if steps.get(k):
            say("   iterate %-10s                                  %s per step" % (names[k], fmt(steps[k], "ms")))
    if all(steps.get(k) for k in legs):
        sa, sp, sc, se = (statistics.median(steps[k]) for k in legs)
        spread = max(max(steps[k]) - min(steps[k]) for k in "pe")
        say("   (a') against (e), same row pointers: %+.4f ms per step, larger spread of the two %.4f ms: %s"
            % (se - sp, spread, "no difference beyond the spread" if abs(se - sp) <= spread else "A DIFFERENCE TO EXPLAIN"))
        say("   the caller's numbering costs %+.4f ms per step against (a); the device order leaves %+.4f ms of it"
            % (sc - sa, se - sa))
        price = statistics.median(wall["e"]) - statistics.median(wall["c"])
        gain = sc - se
        say("   the order costs %.1f ms of set-up, (e) - (c), and takes %+.4f ms off every step%s"
            % (price * 1e3, -gain, ": (e) overtakes (c) after %d iterations" % int(price * 1e3 / gain + 1) if gain > 0 else
               ": (e) never overtakes (c)"))
        saved = statistics.median(wall["a"]) - statistics.median(wall["e"])
        if se - sa > 0:
            say("   (a) takes %.3f s longer to set and is %.4f ms faster per step: it would overtake (e) after %d iterations"
                % (saved, se - sa, int(saved * 1e3 / (se - sa))))
        else:
            say("   (a) takes %.3f s longer to set and is not faster per step (%+.4f ms): it never overtakes (e)" % (saved, sa - se))
    say()
    del ti, tj, tx


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", action="store_true", help="the legs a, a', c, e of the ordered device build (DESIGN.md section 25)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="gl7d19,relat9,relat8")
    args = ap.parse_args()
    os.environ["BLZ_DEVMAT_TRACE"] = "1"
    OUT = open(args.out or os.path.join(ROOT, "profiles", "device_order_cost.txt" if args.order else "device_matrix_cost.txt"), "w")
    if args.order:
        say("tools/device_matrix_cost.py --order on %s: wall seconds of setting the matrix, a a' c e alternated, %d rounds, median "
            "(min .. max);" % (torch.cuda.get_device_name(0), args.rounds))
        say("kernel times from HIP events inside the build (e); iterate: median of %d regions of %d steps" % (REGIONS, STEPS))
        say()
        for name in args.shapes.split(","):
            shape_order(name, args.rounds)
        OUT.close()
        return
    say("tools/device_matrix_cost.py on %s: wall seconds of setting the matrix, a b c d alternated, %d rounds, median (min .. max);"
        % (torch.cuda.get_device_name(0), args.rounds))
    say("kernel times from HIP events inside the build (c); iterate: median of %d regions of %d steps" % (REGIONS, STEPS))
    say()
    for name in args.shapes.split(","):
        shape(name, args.rounds)
    OUT.close()


if __name__ == "__main__":
    main()
