"""What the signed value mode costs per iteration.

    python tools/signed_cost.py [--workload gl7d19] [--steps 20] [--warmup 3] [--repeats 5] [--ns 8,16]

Per block width, two contexts on bench.py's synthetic matrix of the workload, in one process: one unsigned, one in
signed value mode.  At p >= 2^32 the synthetic's words ARE the int32 bit patterns of its values {1,1,1,2,3,-1,-2}, so
both contexts are given the same triplets -- the unsigned one solves for the matrix with 2^32 - 1 and 2^32 - 2 in it, the
signed one for the matrix with -1 and -2; the entries, rows, plan and traffic are the same, the arithmetic per gathered
word is not.  The two are timed in alternation (one region of `steps` iterations each per round, `repeats` rounds,
medians), and the two products alone come from blz_time_kernel.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))


def main():
    import bench
    import blz
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gl7d19", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ns", default="8,16", help="comma-separated block widths")
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    p, right = w["prime"], w["right"]
    assert p >= 1 << 32 and not w["pattern"], "the synthetic's words are bit patterns at 8-byte words only, and it must carry values"
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=False)
    out = dict(workload=args.workload, prime=p, steps=args.steps, repeats=args.repeats, widths={})
    for n in (int(t) for t in args.ns.split(",") if t):
        ctxs = {}
        for kind in ("unsigned", "signed"):
            ctx = blz.Context(p, n)
            if kind == "signed":
                ctx.set_values_signed()
            ctx.set_matrix(M, right)
            ctx.init_v()
            ctxs[kind] = ctx
        assert ctxs["signed"].slab_signed(False) and ctxs["signed"].slab_signed(True)
        assert not ctxs["unsigned"].slab_signed(False) and not ctxs["unsigned"].slab_signed(True)
        plans = {k: [c.plan(t) for t in (False, True)] for k, c in ctxs.items()}
        assert plans["signed"] == plans["unsigned"], "the mode must not change the plan"
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
            forms=[plans["signed"][t]["dot" if plans["signed"][t]["fused"] else "plain"]["form"] for t in (0, 1)],
            fused=[bool(plans["signed"][t]["fused"]) for t in (0, 1)],
            ms_per_step=ms, ms_per_step_all={k: [round(t, 4) for t in v] for k, v in times.items()},
            spread_ms={k: max(v) - min(v) for k, v in times.items()},
            signed_minus_unsigned_ms=ms["signed"] - ms["unsigned"], kernel_ms=kern)
        for ctx in ctxs.values():
            ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
