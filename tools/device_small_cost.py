#!/usr/bin/env python3
"""What the device small algebra costs: HIP events on the caller's stream, medians of five alternated
rounds of a few calls, everything of one section in the same run on the same box.

  1. Context.ortho_coeffs and Context.semi_inverse_device at n = 8, 16, 64 and p = 65537, 2^61 - 1, 2^61 - 31 on a random
     symmetric matrix (full rank: the one-sweep path, which is what an iteration takes), beside the solver's own semi-inverse
     span from blz_profile class 3 over a batch of blz_iterate on a small matrix of the same width and prime.
  2. Context.rref on a full-rank block and on a rank-deficient block (two of its columns repeated and zeroed) of the
     GL7d19-shape row count.
  3. One rebuilt Lanczos step on the relat8-shape and GL7d19-shape stand-ins of bench.py, in three forms: host-free (apply,
     dot, ortho_coeffs, combine: nothing read on the host), with the host round trip of the recipe of
     tests/test_gpu_device_algebra.py (vtAv and vtAAv to the host, the oracle-free numpy-object coefficients there, nested
     lists up again), and blz_iterate itself on a twin context.  Wall-clock per step for the first two (the round trip
     synchronises, events would not see the host's share), the device time blz_iterate reports for the third.

Recorded, not gated.

Usage: tools/device_small_cost.py [--skip-steps]
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

P16, P31, P61, P61B = 65537, (1 << 31) - 1, (1 << 61) - 1, (1 << 61) - 31
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


def medians(calls, rounds=ROUNDS):
    for fn in calls.values():                           # scratch, events, caches: once before the clock
        fn()
    t = {k: [] for k in calls}
    for _ in range(rounds):                             # alternated: every round takes each of them once
        for k, fn in calls.items():
            t[k].append(events(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def solver_semi_inverse_us(p, n):
    """the solver's own semi-inverse kernel, us per launch: blz_profile class 3 over 16 iterations of a small solve"""
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(blz.Matrix.synth(30000, 28000, 300000, 0x534D414C, p))
        ctx.init_v()
        ctx.iterate(4)
        ctx.profile(1)
        done, stopped, _ = ctx.iterate(16)
        span = ctx.profile_read()["semi_inverse"]
        ctx.profile(0)
        assert done == 16 and not stopped and span["launches"] > 0, (done, stopped, span)
        return 1e3 * span["ms_total"] / span["launches"]


def section_chain():
    print("1. the n x n chain: one launch per call, us per call (medians of %d rounds of %d calls); the solver's own" % (ROUNDS, REPS))
    print("   semi-inverse kernel (blz_profile class 3, which also builds its coefficients) beside them")
    print("   and an empty dot (rows = 0: the same checks and two-event ordering around a kernel that does nothing), the floor")
    print("   of a call from Python")
    print("   %-12s %4s %16s %22s %18s %14s" % ("p", "n", "ortho_coeffs", "semi_inverse_device", "solver class 3", "empty dot"))
    for p, pname in ((P16, "65537"), (P61, "2^61 - 1"), (P61B, "2^61 - 31")):
        for n in (8, 16, 64):
            rng = np.random.default_rng([n, 5])
            R = rng.integers(0, p, size=(n, n), dtype=np.uint64).astype(object)
            a, b = up(np.array((R + R.T) % p, dtype=np.uint64)), up(rng.integers(0, p, size=(n, n), dtype=np.uint64))
            with blz.Context(p, n) as ctx:
                out = torch.empty((5, n, n), dtype=torch.uint64, device=DEV)
                none, c = torch.empty((0, n), dtype=torch.int64, device=DEV), torch.empty((n, n), dtype=torch.uint64, device=DEV)
                m = medians({"coef": lambda: ctx.ortho_coeffs(a, b, out=out), "semi": lambda: ctx.semi_inverse_device(a),
                             "floor": lambda: ctx.dot(none, none, out=c)})
                assert int(ctx.ortho_coeffs(a, b)[1].view(torch.int64).cpu()[0]) == n      # (the full-rank path was timed)
            print("   %-12s %4d %13.1f us %19.1f us %15.1f us %11.1f us" % (pname, n, m["coef"], m["semi"], solver_semi_inverse_us(p, n),
                                                                          m["floor"]))


def section_rref(rows):
    print("2. rref of a block of %d rows (the GL7d19 shape), p = 2^61 - 1, us per call" % rows)
    p = P61
    for n in (8, 16):
        g = torch.Generator(device=DEV)
        g.manual_seed(n)
        full = torch.randint(0, p, (rows, n), dtype=torch.int64, device=DEV, generator=g)
        low = full.clone()
        low[:, 1] = low[:, 0]
        low[:, 2] = 0
        with blz.Context(p, n) as ctx:
            m = medians({"full": lambda: ctx.rref(full), "low": lambda: ctx.rref(low), "low_e": lambda: ctx.rref(low, null=False)})
            rf, rl = int(ctx.rref(full)[2][0]), int(ctx.rref(low)[2][0])
        mb = rows * n * 8 / 1e6
        print("   n = %2d: full rank (rank %d, not read whole) %8.1f us;  rank %d (read once, %.1f MB) %8.1f us = %.2f TB/s;  "
              "without z %8.1f us" % (n, rf, m["full"], rl, mb, m["low"], mb / m["low"], m["low_e"]))   # MB / us = TB/s


def host_free_step(ctx, right, v, pb):
    tmp = ctx.apply(not right, v)
    Av = ctx.apply(right, tmp)
    vtAv, vtAAv = ctx.dot(v, Av), ctx.dot(Av, Av)
    coef, _ = ctx.ortho_coeffs(vtAv, vtAAv)
    v2 = ctx.combine([(Av, coef[blz.COEF_V_AV]), (v, coef[blz.COEF_V_V]), (pb, coef[blz.COEF_V_P])])
    p2 = ctx.combine([(pb, coef[blz.COEF_P_P]), (v, coef[blz.COEF_P_V])])
    return v2, p2


def host_step(ctx, right, v, pb, n, p):
    """the recipe of tests/test_gpu_device_algebra.py: the two products to the host, the chain there, nested lists up again
    (Context.semi_inverse_device stands in for the CPU oracle, which a tool does not load; its result is read on the host)"""
    tmp = ctx.apply(not right, v)
    Av = ctx.apply(right, tmp)
    a, b = ctx.dot(v, Av), ctx.dot(Av, Av)
    A1 = a.view(torch.int64).cpu().numpy().view(np.uint64).astype(object)
    A2 = b.view(torch.int64).cpu().numpy().view(np.uint64).astype(object)
    w, d, _ = ctx.semi_inverse_device(a)
    W = w.view(torch.int64).cpu().numpy().view(np.uint64).astype(object)
    nz = d.view(torch.int64).cpu().numpy() != 0
    eye, D = np.eye(n, dtype=object), np.diag(nz.astype(int)).astype(object)
    c = (-(W @ np.where(nz[None, :], A2, A1))) % p
    v2 = ctx.combine([(Av, D.tolist()), (v, ((eye - D) + c) % p), (pb, (-(A1 @ D)) % p)])
    p2 = ctx.combine([(pb, (eye - D).tolist()), (v, W)])
    return v2, p2


def section_steps():
    print("3. one rebuilt Lanczos step, us per step (medians of %d rounds of 8 steps; wall clock between synchronisations for" % ROUNDS)
    print("   the two rebuilt forms, the device time blz_iterate reports for the solver)")
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

            def reset():
                state["v"], state["p"] = v0.clone(), torch.zeros_like(v0)

            def run(step, steps=8):
                reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    state["v"], state["p"] = step(state["v"], state["p"])
                torch.cuda.synchronize()
                return 1e6 * (time.perf_counter() - t0) / steps

            free = lambda: run(lambda v, pb: host_free_step(ctx, right, v, pb))
            host = lambda: run(lambda v, pb: host_step(ctx, right, v, pb, n, p))

            def solver():
                done, stopped, ms = twin.iterate(8)
                assert done == 8 and not stopped
                return 1e3 * ms / 8

            free(), host(), solver()
            t = {"free": [], "host": [], "solver": []}
            for _ in range(ROUNDS):
                t["free"].append(free())
                t["host"].append(host())
                t["solver"].append(solver())
            m = {k: statistics.median(x) for k, x in t.items()}
            print("   %-7s (%d x %d, %d entries, n = %d, p = %d): host-free %9.1f us;  with the host round trip %9.1f us;  "
                  "blz_iterate %9.1f us" % (name, w["rows"], w["cols"], w["nnz"], n, p, m["free"], m["host"], m["solver"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-steps", action="store_true", help="leave out section 3 (the two full-size matrices)")
    args = ap.parse_args()
    section_chain()
    section_rref(WORKLOADS["gl7d19"]["rows"])
    if not args.skip_steps:
        section_steps()


if __name__ == "__main__":
    main()
