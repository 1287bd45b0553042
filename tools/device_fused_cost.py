#!/usr/bin/env python3
"""What the fused device calls cost beside the calls they replace: HIP events on the caller's stream
around ten calls back to back, five alternated rounds, the fused call and its unfused composition in the same process on the
same box.  The composition's kernels are those of the parent commit, byte for byte, so it is the baseline.

  1. Blocks of the GL7d19 row count (1 911 130 rows), p = 2^61 - 1, n = 8 and 16 (and n = 64 at an eighth of the rows):
       dot_pair(v, Av, Av)                      against  dot(v, Av) and dot(Av, Av)
       combine_pair, the update of a step       against  the two combine calls of the seven-call step
     and, at the width of the gl7d19 stand-in, on its matrix:
       apply_pair (no intermediate)             against  two apply calls
     For each: the medians, the composition's min-max spread over its five rounds, and whether
     fused median <= composition median + that spread.
  2. One rebuilt Lanczos step on the relat8-shape and GL7d19-shape stand-ins of bench.py: as four calls (apply_pair,
     dot_pair, ortho_coeffs, combine_pair in place), as seven calls (section 17.1) and as blz_iterate on a twin context.
     Wall clock per step between synchronisations for the rebuilt forms, the device time blz_iterate reports for the third.

Recorded, not gated.

Usage: tools/device_fused_cost.py [--skip-steps]
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

P61 = (1 << 61) - 1
ROUNDS, REPS = 5, 10
DEV = "cuda:0"


def events(fn, reps=REPS):
    """device time of one fn() in us (mean of reps back to back), HIP events on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def alternated(calls, rounds=ROUNDS):
    """{name: the times of its rounds}; every round takes each call once, in turn"""
    for fn in calls.values():                           # scratch, events, caches: once before the clock
        fn()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(events(fn))
    return t


def verdict(what, t):
    fused, comp = statistics.median(t["fused"]), statistics.median(t["composition"])
    spread = max(t["composition"]) - min(t["composition"])
    print("   %-40s fused %8.1f us (min %8.1f max %8.1f);  composition %8.1f us (min %8.1f max %8.1f, spread %6.1f);  %s"
          % (what, fused, min(t["fused"]), max(t["fused"]), comp, min(t["composition"]), max(t["composition"]), spread,
             "met: %.2fx" % (comp / fused) if fused <= comp + spread else "MISSED by %.1f us" % (fused - comp - spread)))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def random_block(rows, n, p, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, p, (rows, n), dtype=torch.int64, device=DEV, generator=g)


def section_calls(rows):
    print("1. the fused calls beside the calls they replace: %d rows, p = 2^61 - 1, us per call (HIP events around %d calls," % (rows, REPS))
    print("   %d alternated rounds).  Criterion: fused median <= composition median + the composition's min-max spread" % ROUNDS)
    p = P61
    for n, rows in ((8, rows), (16, rows), (64, rows // 8)):    # (n = 64: an eighth of the rows, the bytes of n = 8)
        v, Av, pb = (random_block(rows, n, p, 3 * n + k) for k in range(3))
        v2, p2 = torch.empty_like(v), torch.empty_like(v)
        coef = random_block(5 * n, n, p, 99).reshape(5, n, n)
        c2, ca, cb = (torch.empty(s, dtype=torch.uint64, device=DEV) for s in ((2, n, n), (n, n), (n, n)))
        with blz.Context(p, n) as ctx:
            def two_dots():
                ctx.dot(v, Av, out=ca)
                ctx.dot(Av, Av, out=cb)

            def two_combines():
                ctx.combine([(Av, coef[blz.COEF_V_AV]), (v, coef[blz.COEF_V_V]), (pb, coef[blz.COEF_V_P])], out=v2)
                ctx.combine([(pb, coef[blz.COEF_P_P]), (v, coef[blz.COEF_P_V])], out=p2)

            def one_combine():                          # in place on v and p, as a step does it
                ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                                  (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))

            verdict("n = %2d  dot_pair(v, Av, Av)%s" % (n, ", %d rows" % rows if n == 64 else ""),
                    alternated({"fused": lambda: ctx.dot_pair(v, Av, Av, out=c2), "composition": two_dots}))
            verdict("n = %2d  combine_pair, in place" % n, alternated({"fused": one_combine, "composition": two_combines}))


def section_apply():
    w = WORKLOADS["gl7d19"]
    p, n, right = w["prime"], w["n"], w["right"]
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=w["pattern"])
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(M, right)
        xr, yr = ctx.apply_rows(not right)
        x, out = random_block(xr, n, p, 7), torch.empty((xr, n), dtype=torch.uint64, device=DEV)
        mid = torch.empty((yr, n), dtype=torch.uint64, device=DEV)

        def two_applies():
            ctx.apply(not right, x, out=mid)
            ctx.apply(right, mid, out=out)

        verdict("n = %2d  apply_pair on gl7d19" % n, alternated({"fused": lambda: ctx.apply_pair(not right, x, out=out),
                                                                 "composition": two_applies}))
        verdict("n = %2d  apply_pair with mid" % n, alternated({"fused": lambda: ctx.apply_pair(not right, x, out=out, mid=mid),
                                                                "composition": two_applies}))


def seven_calls(ctx, right, v, pb):
    tmp = ctx.apply(not right, v)
    Av = ctx.apply(right, tmp)
    vtAv, vtAAv = ctx.dot(v, Av), ctx.dot(Av, Av)
    coef, _ = ctx.ortho_coeffs(vtAv, vtAAv)
    v2 = ctx.combine([(Av, coef[blz.COEF_V_AV]), (v, coef[blz.COEF_V_V]), (pb, coef[blz.COEF_V_P])])
    p2 = ctx.combine([(pb, coef[blz.COEF_P_P]), (v, coef[blz.COEF_P_V])])
    return v2, p2


def four_calls(ctx, right, v, pb):
    Av = ctx.apply_pair(not right, v)
    c = ctx.dot_pair(v, Av, Av)
    coef, _ = ctx.ortho_coeffs(c[0], c[1])
    ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))
    return v, pb


def section_steps():
    print("2. one rebuilt Lanczos step, us per step (medians of %d alternated rounds of 8 steps, min and max beside them; wall" % ROUNDS)
    print("   clock between synchronisations for the rebuilt forms, the device time blz_iterate reports for the solver)")
    for name in ("relat8", "gl7d19"):
        w = WORKLOADS[name]
        p, n, right = w["prime"], w["n"], w["right"]
        M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=w["pattern"])
        with blz.Context(p, n) as ctx, blz.Context(p, n) as twin:
            ctx.set_matrix(M, right)
            twin.set_matrix(M, right)
            twin.init_v()
            rows = twin.rows(blz.V)
            v0 = up(twin.get_block(blz.V).reshape(rows, n))
            state = {}

            def run(step, steps=8):
                state["v"], state["p"] = v0.clone(), torch.zeros_like(v0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    state["v"], state["p"] = step(ctx, right, state["v"], state["p"])
                torch.cuda.synchronize()
                return 1e6 * (time.perf_counter() - t0) / steps

            def solver():
                done, stopped, ms = twin.iterate(8)
                assert done == 8 and not stopped
                return 1e3 * ms / 8

            forms = {"four": lambda: run(four_calls), "seven": lambda: run(seven_calls), "solver": solver}
            for fn in forms.values():
                fn()
            run(four_calls)                             # the two forms walk the same path
            b = state["v"].clone().view(torch.int64)
            run(seven_calls)
            assert torch.equal(b, state["v"].view(torch.int64)), "four calls and seven calls disagree"
            t = {k: [] for k in forms}
            for _ in range(ROUNDS):
                for k, fn in forms.items():
                    t[k].append(fn())
            show = lambda k: "%9.1f us (%.1f .. %.1f)" % (statistics.median(t[k]), min(t[k]), max(t[k]))
            print("   %-7s (%d x %d, %d entries, n = %d, p = %d):\n           four calls %s;  seven calls %s;  blz_iterate %s"
                  % (name, w["rows"], w["cols"], w["nnz"], n, p, show("four"), show("seven"), show("solver")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-steps", action="store_true", help="leave out apply_pair and section 2 (the two full-size matrices)")
    args = ap.parse_args()
    section_calls(WORKLOADS["gl7d19"]["rows"])
    if not args.skip_steps:
        section_apply()
        section_steps()


if __name__ == "__main__":
    main()
