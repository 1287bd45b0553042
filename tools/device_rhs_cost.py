#!/usr/bin/env python3
"""What the two ends of M x = b cost, through the host and on the device.

Shapes: the GL7d19 and relat8 shapes of bench.py, triplets from Matrix.synth, n = 8, p = 2^61 - 1 and 2^31 - 1, k = 1 and 8
right-hand sides.  Per shape, prime and k, ONE context whose matrix is set on the host with the k empty border lines (the
default renumbering: the gather and the scatter of the new kernels go through a real permutation), and on it, wall time of
  (A) set_rhs_block from a numpy block on the host      against  (B) set_rhs_device from a tensor resident on the GPU;
  (A) solution_block into a numpy block                 against  (B) solution_device into a tensor on the GPU,
the solution calls on the state of one short solve that was stopped after STEPS steps: before every timed call V and TMP are
put back from device copies (not timed), so every call reduces the same blocks.  Such a block solves no system: the statuses
are 1, x is zeros -- and both forms move every word they would move for a solved one (the whole V block to the host and the
loop over its rows; the export kernel).  Alternated A B A B, ROUNDS rounds, a figure is the median with its min .. max.

Recorded, not gated.  There is no CPU path: without a GPU this fails.

Usage: tools/device_rhs_cost.py [--out profiles/device_rhs_cost.txt] [--rounds 5] [--shapes gl7d19,relat8]
One process, one GPU step: run it under a time limit of its own and chain whatever follows with `&&`.  The table is written
line by line as it is measured.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))
sys.path.insert(0, ROOT)
import blz  # noqa: E402
from bench import WORKLOADS  # noqa: E402

DEV = "cuda:0"
N, STEPS = 8, 6
PRIMES = ((1 << 61) - 1, (1 << 31) - 1)
KS = (1, 8)
OUT = None


def say(line=""):
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def fmt(ts):
    return "%9.3f ms (%9.3f .. %9.3f)" % (statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3)


def timed(ctx, call):
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    out = call()
    ctx.sync()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def case(M, w, p, k, rounds):
    right = w["right"]
    Mk = blz.Matrix(M.nrows + (0 if right else k), M.ncols + (k if right else 0), M.i, M.j, M.x)
    with blz.Context(p, N) as ctx:
        ctx.set_matrix(Mk, right)
        length, xrows = ctx.rows(blz.TMP), ctx.rows(blz.V) - k
        rng = np.random.default_rng(k)
        hb = (rng.integers(0, 1 << 62, size=(length, k), dtype=np.uint64) % np.uint64(p)).astype(np.uint64)
        db = torch.from_numpy(hb.view(np.int64)).to(DEV)
        wall = {key: [] for key in ("set A", "set B", "sol A", "sol B")}
        for _ in range(rounds):
            wall["set A"].append(timed(ctx, lambda: ctx.set_rhs_block(hb))[0])
            wall["set B"].append(timed(ctx, lambda: ctx.set_rhs_device(db))[0])
        ctx.init_v()
        ctx.iterate(STEPS)
        v0, t0 = ctx.get_block_device(blz.V), ctx.get_block_device(blz.TMP)
        xd = torch.zeros((xrows, k), dtype=torch.int64, device=DEV)
        status = {}
        for _ in range(rounds):
            for key, call in (("sol A", ctx.solution_block), ("sol B", lambda: ctx.solution_device(out=xd))):
                ctx.set_block_device(blz.V, v0)
                ctx.set_block_device(blz.TMP, t0)
                dt, (st, _) = timed(ctx, call)
                wall[key].append(dt)
                status[key] = st
        assert status["sol A"] == status["sol B"], status
        say("   k = %d: b %d x %d (%.1f MB as u64), x %d x %d, V block %.1f MB; statuses %s"
            % (k, length, k, length * k * 8e-6, xrows, k, ctx.rows(blz.V) * N * 8e-6, status["sol B"]))
        say("      (A) set_rhs_block, host b            %s" % fmt(wall["set A"]))
        say("      (B) set_rhs_device, resident b       %s" % fmt(wall["set B"]))
        say("      (A) solution_block, host x           %s" % fmt(wall["sol A"]))
        say("      (B) solution_device, resident x      %s" % fmt(wall["sol B"]))
        del v0, t0, xd, db


def shape(name, rounds):
    w = WORKLOADS[name]
    for p in PRIMES:
        M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, w["pattern"])
        say("%s: %d x %d, %d entries, n = %d, p = %d, %s" % (w["desc"], M.nrows, M.ncols, M.nnz, N, p,
                                                             "M x = b" if w["right"] else "x M = b"))
        for k in KS:
            case(M, w, p, k, rounds)
        say()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_rhs_cost.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="gl7d19,relat8")
    args = ap.parse_args()
    OUT = open(args.out, "w")
    say("tools/device_rhs_cost.py on %s: wall milliseconds of setting the right-hand sides and of reading the solution, A B"
        % torch.cuda.get_device_name(0))
    say("alternated, %d rounds, median (min .. max); the solution calls on the blocks of a solve stopped after %d steps"
        % (args.rounds, STEPS))
    say()
    for name in args.shapes.split(","):
        shape(name, args.rounds)
    OUT.close()


if __name__ == "__main__":
    main()
