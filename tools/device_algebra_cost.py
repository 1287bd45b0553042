#!/usr/bin/env python3
"""What the device block algebra costs: Context.dot and Context.combine on blocks of the GL7d19-shape row
count (1 911 130 rows), p = 2^61 - 1 and p = 65537, n = 8 and n = 16, HIP events on the caller's stream, medians of five
alternated rounds -- against, on the same box in the same run,

  - the solver's own vector-ALU kernels on its slabs through blz_time_kernel on a context made with BLZ_NO_MFMA=1:
    which = 2, the inner products (v^T Av and Av^T Av in ONE pass over two blocks), and which = 3, the block update (reads
    three blocks, writes two).  Their slabs hold words of blz_word_bytes: 4 bytes at p = 65537, where a caller's block
    always has 8-byte words and so moves twice the bytes;
  - the same two on the matrix cores (p = 2^61 - 1 only, a default context), for the record;
  - the 6.3 TB/s streaming ceiling of profiles/r02_ubench3_streaming_ceiling.txt.

Per call: bytes moved, microseconds, TB/s.  Recorded, not gated.  The matrix only gives the solver's slabs their row count: a
sparse synthetic (two entries per row) is enough, none of the kernels timed here reads it.

Usage: tools/device_algebra_cost.py [--rows R]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))
import blz  # noqa: E402

P61, P16 = (1 << 61) - 1, 65537
ROUNDS, REPS = 5, 3
CEILING = 6.3e12        # bytes/s, copy of 122 MB arrays (profiles/r02_ubench3_streaming_ceiling.txt)


def events(fn):
    """device time of one fn() in ms (mean of REPS back to back), HIP events on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def line(tag, ms, nbytes):
    rate = nbytes / (ms * 1e-3)
    print(f"    {tag:<58s} {nbytes / 1e6:7.1f} MB  {ms * 1e3:8.1f} us  {rate / 1e12:5.2f} TB/s = {100 * rate / CEILING:3.0f} % of the ceiling")
    return rate


def solver_context(M, p, n, no_mfma):
    if no_mfma:
        os.environ["BLZ_NO_MFMA"] = "1"                 # read by blz_create
    try:
        ctx = blz.Context(p, n)
    finally:
        os.environ.pop("BLZ_NO_MFMA", None)
    ctx.set_matrix(M)
    ctx.init_v()
    done, stopped, _ = ctx.iterate(2)                   # valid coefficients, the stop flag down: the kernels do their work
    assert done == 2 and not stopped
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1911130)
    args = ap.parse_args()
    rows = args.rows
    print(f"blocks of {rows} rows (the GL7d19 shape), medians of {ROUNDS} alternated rounds of {REPS} calls, HIP events; "
          f"ceiling {CEILING / 1e12:.1f} TB/s")
    for p, pname in ((P61, "2^61 - 1"), (P16, "65537")):
        M = blz.Matrix.synth(rows, rows + 44179, 2 * rows, 0x474C3764, p)
        for n in (8, 16):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(n)
            v, av, pb = (torch.randint(0, p, (rows, n), dtype=torch.int64, device="cuda:0", generator=g) for _ in range(3))
            coef = [torch.randint(0, p, (n, n), dtype=torch.int64, device="cuda:0", generator=g) for _ in range(3)]
            out = torch.empty_like(v)
            c = torch.empty((n, n), dtype=torch.int64, device="cuda:0")
            blk = rows * n * 8
            par = solver_context(M, p, n, no_mfma=True)
            mfma = solver_context(M, p, n, no_mfma=False) if p == P61 else None
            assert par.rows(blz.V) == rows
            pblk = rows * par.plan(False)["width"] * par.word_bytes     # a slab: the width in HBM, the solver's word
            calls = {
                "dot_xy": lambda: par.dot(v, av, out=c),
                "dot_xx": lambda: par.dot(av, av, out=c),
                "comb3": lambda: par.combine([(av, coef[0]), (v, coef[1]), (pb, coef[2])], out=out),
                "comb2": lambda: par.combine([(pb, coef[0]), (v, coef[1])], out=out),
                "comb2_inplace": lambda: par.combine([(out, coef[0]), (v, coef[1])], out=out),
                "par_dot": None, "par_upd": None, "mfma_dot": None, "mfma_upd": None,
            }
            for fn in calls.values():                   # scratch, events, caches: once before the clock
                if fn:
                    fn()
            t = {k: [] for k in calls}
            for _ in range(ROUNDS):                     # alternated: every round takes each of them once
                for k, fn in calls.items():
                    if fn:
                        t[k].append(events(fn))
                t["par_dot"].append(par.time_kernel(2, REPS))
                t["par_upd"].append(par.time_kernel(3, REPS))
                if mfma:
                    t["mfma_dot"].append(mfma.time_kernel(2, REPS))
                    t["mfma_upd"].append(mfma.time_kernel(3, REPS))
            m = {k: statistics.median(x) for k, x in t.items() if x}
            print(f"p = {pname}, n = {n}: a caller's block is {blk / 1e6:.1f} MB (8-byte words), a slab of the solver "
                  f"{pblk / 1e6:.1f} MB ({par.word_bytes}-byte words)")
            print("  inner products")
            r1 = line("dot(v, Av): reads 2 blocks", m["dot_xy"], 2 * blk)
            line("dot(Av, Av), the Gram form: reads 1 block", m["dot_xx"], blk)
            r0 = line("solver, vector ALU (which = 2): both products, reads 2 slabs", m["par_dot"], 2 * pblk)
            if mfma:
                line("solver, matrix cores (which = 2)", m["mfma_dot"], 2 * pblk)
            print(f"    both products: device calls {1e3 * (m['dot_xy'] + m['dot_xx']):.1f} us, solver's vector-ALU kernel "
                  f"{1e3 * m['par_dot']:.1f} us; bytes per second, dot(v, Av) / solver = {r1 / r0:.2f}")
            print("  recombination")
            r3 = line("combine, 3 terms (v'): reads 3 blocks, writes 1", m["comb3"], 4 * blk)
            line("combine, 2 terms (p'): reads 2 blocks, writes 1", m["comb2"], 3 * blk)
            line("combine, 2 terms, in place", m["comb2_inplace"], 3 * blk)
            ru = line("solver, vector ALU (which = 3): v' and p', reads 3 slabs, writes 2", m["par_upd"], 5 * pblk)
            if mfma:
                line("solver, matrix cores (which = 3)", m["mfma_upd"], 5 * pblk)
            print(f"    v' and p': device calls {1e3 * (m['comb3'] + m['comb2']):.1f} us, solver's vector-ALU kernel "
                  f"{1e3 * m['par_upd']:.1f} us; bytes per second, 3-term combine / solver = {r3 / ru:.2f}")
            par.close()
            if mfma:
                mfma.close()


if __name__ == "__main__":
    main()
