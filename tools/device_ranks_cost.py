#!/usr/bin/env python3
"""What device blocks on ranks cost, on the GL7d19-shape synthetic, p = 2^61 - 1, n = 8, left kernel.
HIP events on the caller's stream, medians of five alternated rounds of three calls.  Recorded, not gated.

(a) rank-local apply against apply with the mode off, on one plain rank and the same context: the blocks are then the same
    rows in two numberings, and the difference is what the permutation of the import and the export costs.
(b) dot and dot_pair with the collective forced on (a one-rank loopback group under BLZ_FORCE_COMM=1: the send buffer, the
    all-reduce and the kernel that reduces the sums) against a plain context.
(c) the four-call step (apply_pair, dot_pair, ortho_coeffs, combine_pair) on 2 loopback ranks against one plain rank.

Loopback ranks are threads of one process that SHARE one device: two of them split the rows and then run on the same CUs, so
(c) shows the overhead of the exchange and of the rendezvous, not scaling.  No run on more than one GPU exists.

Usage: tools/device_ranks_cost.py [--rows R --cols C --nnz NNZ]   (default: the GL7d19 shape of bench.py)
"""
import argparse
import os
import statistics
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python"))
import blz  # noqa: E402

P61 = (1 << 61) - 1
ROUNDS, REPS = 5, 3
DEV = "cuda:0"


def events(fn, stream=None):
    """device time of one fn() in ms (mean of REPS back to back), HIP events on the given (or torch's current) stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / REPS


def block(rows, n, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, P61, (rows, n), dtype=torch.int64, device=DEV, generator=g)


def alternated(calls):
    """{name: median ms} of ROUNDS rounds that take every call once"""
    for fn in calls.values():           # scratch, events, caches: once before the clock
        fn()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t[k].append(events(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def step(ctx, right, v, pb, stream=None):
    Av = ctx.apply_pair(not right, v, stream=stream)
    c = ctx.dot_pair(v, Av, Av, stream=stream)
    coef, _ = ctx.ortho_coeffs(c[0], c[1], stream=stream)
    ctx.combine_pair([(Av, coef[blz.COEF_V_AV], None), (v, coef[blz.COEF_V_V], coef[blz.COEF_P_V]),
                      (pb, coef[blz.COEF_V_P], coef[blz.COEF_P_P])], out=(v, pb), stream=stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1911130)
    ap.add_argument("--cols", type=int, default=1955309)
    ap.add_argument("--nnz", type=int, default=37322725)
    args = ap.parse_args()
    n, right = 8, False
    M = blz.Matrix.synth(args.rows, args.cols, args.nnz, 0x474C3764, P61)
    print(f"matrix {M.nrows} x {M.ncols}, {M.nnz} entries (GL7d19-shape synthetic), p = 2^61 - 1, n = {n}, left kernel; "
          f"medians of {ROUNDS} alternated rounds of {REPS} calls, HIP events")

    # (a) and the one-rank side of (b) and (c): one plain context
    with blz.Context(P61, n) as ctx:
        ctx.set_matrix(M, right)
        calls = {}
        for t in (True, False):
            xr, yr = ctx.apply_rows(t)
            x, y = block(xr, n, 1 + int(t)), torch.empty((yr, n), dtype=torch.int64, device=DEV)
            calls[("off", t)] = lambda t=t, x=x, y=y: ctx.device_ranks(False).apply(t, x, out=y)
            calls[("on", t)] = lambda t=t, x=x, y=y: ctx.device_ranks(True).apply(t, x, out=y)
        m = alternated(calls)
        print("(a) apply on one plain rank: the mode off (rows in the file's numbering, permuted on the way in and out) "
              "against the mode on (slab order)")
        for t in (True, False):
            off, on = m[("off", t)], m[("on", t)]
            print(f"    {'M^T x' if t else 'M x  '}   mode off {off * 1e3:7.1f} us   mode on {on * 1e3:7.1f} us   "
                  f"the permutation {1e3 * (off - on):6.1f} us = {100 * (off - on) / off:.0f} % of the call with the mode off")
        ctx.device_ranks(False)
        rows = ctx.rows(blz.V)
        v, av = block(rows, n, 5), block(rows, n, 6)
        plain = alternated({"dot": lambda: ctx.dot(v, av), "dot_pair": lambda: ctx.dot_pair(v, av, av)})
        v1, p1 = block(rows, n, 7), torch.zeros((rows, n), dtype=torch.int64, device=DEV)
        one = alternated({"step": lambda: step(ctx, right, v1, p1)})["step"]

    # (b) the collective forced on: one rank, a loopback group, BLZ_FORCE_COMM=1 (read when the communicator is attached)
    os.environ["BLZ_FORCE_COMM"] = "1"
    group = blz.LoopGroup(1)
    try:
        with blz.Context(P61, n) as ctx:
            ctx.comm_init_loopback(group, 0)
            ctx.device_ranks()
            forced = alternated({"dot": lambda: ctx.dot(v, av), "dot_pair": lambda: ctx.dot_pair(v, av, av)})
    finally:
        os.environ.pop("BLZ_FORCE_COMM", None)
        group.close()
    print(f"(b) inner products of blocks of {rows} rows: a plain context against one rank with the collective forced on")
    for k in ("dot", "dot_pair"):
        print(f"    {k:<9s} plain {plain[k] * 1e3:7.1f} us   collective {forced[k] * 1e3:7.1f} us   "
              f"send buffer + all-reduce + reduction {1e3 * (forced[k] - plain[k]):6.1f} us")
    del v, av

    # (c) the four-call step on 2 loopback ranks: a thread and a stream per rank, the rounds in step
    nranks = 2
    group = blz.LoopGroup(nranks)
    seed = blz.Context(P61, n)
    P = blz.Prepared.prepare_for(seed, M, right, nranks)
    seed.close()
    times, errs = [[] for _ in range(nranks)], [None] * nranks
    shares = [0] * nranks

    def rank_main(g):
        try:
            s = torch.cuda.Stream(device=DEV)
            with blz.Context(P61, n) as ctx, torch.cuda.stream(s):
                ctx.comm_init_loopback(group, g)
                ctx.device_ranks()
                ctx.set_matrix_prepared(P, g)
                shares[g] = ctx.local_rows(blz.V)[1]
                vg = block(shares[g], n, 10 + g)
                pg = torch.zeros_like(vg)
                step(ctx, right, vg, pg, s)
                for _ in range(ROUNDS):
                    times[g].append(events(lambda: step(ctx, right, vg, pg, s), s))
                ctx.sync()
        except BaseException as e:      # noqa: BLE001 (reported below)
            errs[g] = e

    ths = [threading.Thread(target=rank_main, args=(g,)) for g in range(nranks)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    P.close()
    group.close()
    for e in errs:
        if e is not None:
            raise e
    two = [statistics.median(t) for t in times]
    print(f"(c) the four-call step: one plain rank ({rows} rows of v) {one * 1e3:7.1f} us; 2 loopback ranks "
          f"({shares[0]} + {shares[1]} rows) " + ", ".join(f"rank {g} {ms * 1e3:7.1f} us" for g, ms in enumerate(two)))
    print(f"    2 ranks / 1 rank = {max(two) / one:.2f}.  The two ranks share ONE device: they split the rows and run on the same "
          "CUs, so this is the overhead of the exchange and the rendezvous, not scaling; no run on more than one GPU exists.")


if __name__ == "__main__":
    main()
