"""What wide matrix entries cost per iteration.

    python tools/wide_cost.py [--workload gl7d19] [--steps 20] [--warmup 3] [--repeats 5] [--ns 8,16] [--primes 61f,61b]

Per prime (2^61 - 1: x' is a rotation; 2^61 - 31: x' is a Barrett reduction) and block width, three contexts on the
structure of bench.py's synthetic matrix of the workload, in one process:
    u32      today's values {1,1,1,2,3,-1,-2} as u32 words in a value array (BLZ_NO_PACK=1 while it is set)
    array    uniform residues below p in val + val_hi (more than 256 distinct: no palette)
    palette  seven residues of full width through the packed stream and its two LDS tables
The three are timed in alternation (one region of `steps` iterations each per round, `repeats` rounds, medians), and the
two products alone come from blz_time_kernel.  Prints one JSON line per prime.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))

PRIMES = {"61f": (1 << 61) - 1, "61b": (1 << 61) - 31}


def main():
    import bench
    import blz
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gl7d19", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ns", default="8,16", help="comma-separated block widths")
    ap.add_argument("--primes", default="61f,61b", help="comma-separated: 61f = 2^61 - 1, 61b = 2^61 - 31")
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    right = w["right"]
    for pname in (t for t in args.primes.split(",") if t):
        p = PRIMES[pname]
        S = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=False)
        rng = np.random.default_rng(w["seed"])
        uniform = rng.integers(0, p, size=S.nnz, dtype=np.int64)
        seven = np.array([p - 1, p - 2, (1 << 32) + 1, p - (1 << 32), p >> 1, (p >> 1) + 3, 0x1234567 << 32], dtype=np.int64)
        few = seven[rng.integers(0, 7, size=S.nnz)]
        mats = {"u32": S}
        for kind, x in (("array", uniform), ("palette", few)):
            mats[kind] = blz.Matrix(S.nrows, S.ncols, S.i, S.j, (x & 0xFFFFFFFF).astype(np.uint32), x_hi=(x >> 32).astype(np.uint32))
        out = dict(workload=args.workload, prime=p, steps=args.steps, repeats=args.repeats, widths={})
        for n in (int(t) for t in args.ns.split(",") if t):
            ctxs = {}
            for kind, M in mats.items():
                if kind == "u32":
                    os.environ["BLZ_NO_PACK"] = "1"     # read when the context is created
                ctx = blz.Context(p, n)
                os.environ.pop("BLZ_NO_PACK", None)
                ctx.set_matrix(M, right)
                ctx.init_v()
                ctxs[kind] = ctx
            plans = {k: [c.plan(t) for t in (False, True)] for k, c in ctxs.items()}
            assert all(ctxs[k].slab_wide(t) for k in ("array", "palette") for t in (False, True))
            assert not ctxs["u32"].slab_wide(False) and not ctxs["u32"].slab_wide(True)
            assert [plans["u32"][t]["packed"] for t in (0, 1)] == [2, 2] and [plans["array"][t]["packed"] for t in (0, 1)] == [2, 2]
            assert [plans["palette"][t]["packed"] for t in (0, 1)] == [1, 1]
            for ctx in ctxs.values():
                done, stopped, _ = ctx.iterate(args.warmup)
                assert done == args.warmup and not stopped
            times = {k: [] for k in ctxs}
            for _ in range(args.repeats):
                for k, ctx in ctxs.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    done, stopped, _ = ctx.iterate(args.steps)
                    ctx.sync()
                    times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
                    assert done == args.steps and not stopped
            ms = {k: statistics.median(v) for k, v in times.items()}
            kern = {k: {name: ctxs[k].time_kernel(which, 20) for which, name in ((0, "spmv1"), (1, "spmv2"))} for k in ctxs}
            out["widths"][str(n)] = dict(
                forms={k: [plans[k][t]["dot" if plans[k][t]["fused"] else "plain"]["form"] for t in (0, 1)] for k in ctxs},
                fused={k: [bool(plans[k][t]["fused"]) for t in (0, 1)] for k in ctxs},
                stream_bytes={k: [ctxs[k].matrix_stream_bytes(t) for t in (False, True)] for k in ctxs},
                ms_per_step=ms, ms_per_step_all={k: [round(t, 4) for t in v] for k, v in times.items()},
                spread_ms={k: max(v) - min(v) for k, v in times.items()},
                array_minus_u32_ms=ms["array"] - ms["u32"], palette_minus_u32_ms=ms["palette"] - ms["u32"], kernel_ms=kern)
            for ctx in ctxs.values():
                ctx.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
