#!/usr/bin/env python3
"""What the device block algebra costs on the matrix cores beside the vector-ALU kernels it replaces:
two contexts in one process -- one created under BLZ_NO_MFMA=1, whose device calls run the vector-ALU kernels of blz_devalg.hip
(the baseline), one created under
BLZ_DEV_MFMA_MIN_ROWS=0, whose calls take the forms of blz_devmfma.hip at every row count -- the same calls on the same blocks,
alternated.  HIP events on the caller's stream around ten calls back to back, five rounds; medians with min and max.

  1. p = 2^61 - 1, n = 8 and 16, rows 2^12, 2^14, 2^16, 2^18, 2^20 and 1 911 130 (the GL7d19 row count):
       dot(v, Av)    dot_pair(v, Av, Av)    combine of 2 and of 3 terms    combine_pair in place (the update of a step)
     A form counts as FASTER at a row count when its median <= the baseline's median minus the baseline's min-max spread.
     The default threshold of a (call, width) is the smallest measured row count from which the form is faster at every
     larger one; "off" where there is none (the form stays reachable with BLZ_DEV_MFMA_MIN_ROWS).
  2. One Lanczos step rebuilt from four calls (apply_pair, dot_pair, ortho_coeffs, combine_pair in place) on the GL7d19-shape
     stand-in of bench.py at n = 8, with the forms on and off, beside blz_iterate on a twin context.

Recorded, not gated.  Not measured here: what binds the new kernels (no counter run), strided blocks (ld > n) at scale, and
widths other than 8 and 16 (which have no matrix-core form).

Usage: tools/device_mfma_cost.py [--skip-step] [--out FILE]      (default FILE: profiles/device_mfma_cost.txt)
"""
import argparse
import contextlib
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
ROWS = (1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, WORKLOADS["gl7d19"]["rows"])
CALLS = ("dot", "dot_pair", "combine2", "combine3", "combine_pair")
KIND = {"dot": "dot", "dot_pair": "dot_pair", "combine2": "combine", "combine3": "combine", "combine_pair": "combine_pair"}
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def contexts(n, st):
    """(forms on at every row count, baseline)"""
    with environment(BLZ_DEV_MFMA_MIN_ROWS="0", BLZ_NO_MFMA=None):
        on = st.enter_context(blz.Context(P61, n))
    with environment(BLZ_DEV_MFMA_MIN_ROWS=None, BLZ_NO_MFMA="1"):
        off = st.enter_context(blz.Context(P61, n))
    return on, off


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
    for fn in calls.values():                           # scratch, events, caches: once before the clock
        fn()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(events(fn))
    return t


def random_block(rows, n, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, P61, (rows, n), dtype=torch.int64, device=DEV, generator=g)


def calls_of(ctx, n, v, Av, pb, z, coef, c1, c2):
    return {"dot": lambda: ctx.dot(v, Av, out=c1),
            "dot_pair": lambda: ctx.dot_pair(v, Av, Av, out=c2),
            "combine2": lambda: ctx.combine([(pb, coef[blz.COEF_P_P]), (v, coef[blz.COEF_P_V])], out=z),
            "combine3": lambda: ctx.combine([(Av, coef[blz.COEF_V_AV]), (v, coef[blz.COEF_V_V]), (pb, coef[blz.COEF_V_P])], out=z),
            "combine_pair": lambda: ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                                                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))}


def section_calls():
    say("1. the matrix-core forms beside the vector-ALU kernels: p = 2^61 - 1, us per call (HIP events around %d calls, %d" % (REPS, ROUNDS))
    say("   alternated rounds; median, min .. max).  FASTER: form median <= baseline median - the baseline's min-max spread")
    faster = {}
    for n in (8, 16):
        with contextlib.ExitStack() as st:
            on, off = contexts(n, st)
            op = {"dot": blz.DEVOP_DOT, "dot_pair": blz.DEVOP_DOT_PAIR, "combine": blz.DEVOP_COMBINE, "combine_pair": blz.DEVOP_COMBINE_PAIR}
            for rows in ROWS:
                v, Av, pb = (random_block(rows, n, 3 * n + k) for k in range(3))
                z = torch.empty_like(v)
                coef = random_block(5 * n, n, 99).reshape(5, n, n)
                c1, c2 = (torch.empty(s, dtype=torch.uint64, device=DEV) for s in ((n, n), (2, n, n)))
                f_on, f_off = calls_of(on, n, v, Av, pb, z, coef, c1, c2), calls_of(off, n, v, Av, pb, z, coef, c1, c2)
                for name in CALLS:
                    nterms = {"combine2": 2, "combine3": 3, "combine_pair": 3}.get(name, 1)
                    assert on.devalg_plan(op[KIND[name]], rows, nterms)["form"] == 1
                    assert off.devalg_plan(op[KIND[name]], rows, nterms)["form"] == 0
                    t = alternated({"form": f_on[name], "baseline": f_off[name]})
                    fm, bm = statistics.median(t["form"]), statistics.median(t["baseline"])
                    spread = max(t["baseline"]) - min(t["baseline"])
                    ok = fm <= bm - spread
                    faster[(name, n, rows)] = ok
                    say("   n = %2d  %-12s %8d rows   matrix cores %8.1f us (%8.1f .. %8.1f)   vector ALU %8.1f us (%8.1f .. %8.1f, spread %6.1f)   %s"
                        % (n, name, rows, fm, min(t["form"]), max(t["form"]), bm, min(t["baseline"]), max(t["baseline"]), spread,
                           "FASTER %.2fx" % (bm / fm) if ok else "not faster (%.2fx)" % (bm / fm)))
                del v, Av, pb, z
    say()
    say("   default thresholds by the criterion (smallest measured row count from which the form is faster at every larger one):")
    for kind in ("dot", "dot_pair", "combine", "combine_pair"):
        for n in (8, 16):
            names = [c for c in CALLS if KIND[c] == kind]
            thr = None
            for rows in reversed(ROWS):
                if all(faster[(c, n, rows)] for c in names):
                    thr = rows
                else:
                    break
            say("   %-12s n = %2d   %s" % (kind, n, "%d rows" % thr if thr is not None else "off (no such row count)"))


def four_calls(ctx, right, v, pb):
    Av = ctx.apply_pair(not right, v)
    c = ctx.dot_pair(v, Av, Av)
    coef, _ = ctx.ortho_coeffs(c[0], c[1])
    ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb))
    return v, pb


def section_step():
    say()
    say("2. one Lanczos step rebuilt from four calls on the GL7d19 shape, us per step (medians of %d alternated rounds of 8 steps," % ROUNDS)
    say("   min .. max; wall clock between synchronisations for the rebuilt forms, the device time blz_iterate reports for the solver)")
    w = WORKLOADS["gl7d19"]
    p, n, right = w["prime"], w["n"], w["right"]
    assert p == P61 and n == 8
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], p, pattern=w["pattern"])
    with contextlib.ExitStack() as st:
        on, off = contexts(n, st)
        twin = st.enter_context(blz.Context(p, n))
        for c in (on, off, twin):
            c.set_matrix(M, right)
        twin.init_v()
        rows = twin.rows(blz.V)
        v0 = torch.from_numpy(np.ascontiguousarray(twin.get_block(blz.V).reshape(rows, n)).view(np.int64)).to(DEV)
        state = {}

        def run(ctx, steps=8):
            state["v"], state["p"] = v0.clone(), torch.zeros_like(v0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                four_calls(ctx, right, state["v"], state["p"])
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0) / steps

        def solver():
            done, stopped, ms = twin.iterate(8)
            assert done == 8 and not stopped
            return 1e3 * ms / 8

        forms = {"matrix cores": lambda: run(on), "vector ALU": lambda: run(off), "blz_iterate": solver}
        for fn in forms.values():
            fn()
        run(on)                                         # the two forms write the same words
        b = state["v"].clone().view(torch.int64)
        run(off)
        assert torch.equal(b, state["v"].view(torch.int64)), "the two forms disagree"
        t = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, fn in forms.items():
                t[k].append(fn())
        for k in forms:
            say("   %-14s %9.1f us (%.1f .. %.1f)" % (k, statistics.median(t[k]), min(t[k]), max(t[k])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true", help="leave out section 2 (the full-size matrix)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_mfma_cost.txt"))
    args = ap.parse_args()
    say("tools/device_mfma_cost.py on %s" % torch.cuda.get_device_name(0))
    section_calls()
    if not args.skip_step:
        section_step()
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
