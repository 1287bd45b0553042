#!/usr/bin/env python3
"""What device blocks cost, on the GL7d19-shape synthetic, p = 2^61 - 1, n = 8 and n = 16.

(a) the host path as the yardstick: blz_set_block + blz_get_block of V (a copy each way and the CPU's renumbering) against
    set_block_device + get_block_device of the same block, medians of five alternated rounds; and the two kernels alone
    (HIP events on the caller's stream around a call each), as achieved bytes/s beside the streaming ceiling of
    profiles/r02_ubench3_streaming_ceiling.txt (copy of 122 MB arrays: 6.3 TB/s).
(b) the overhead of apply: Context.apply (import + product + export) against blz_time_kernel's figure for the same product
    alone; the difference is the two passes.

Usage: tools/device_blocks_cost.py [--rows R --cols C --nnz NNZ]   (default: the GL7d19 shape of bench.py)
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
import blz  # noqa: E402

P61 = (1 << 61) - 1
ROUNDS = 5
CEILING = 6.3e12        # bytes/s, copy of 122 MB arrays (profiles/r02_ubench3_streaming_ceiling.txt)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def events(fn, reps=5):
    """median device time of fn() in ms, HIP events on torch's current stream"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1911130)
    ap.add_argument("--cols", type=int, default=1955309)
    ap.add_argument("--nnz", type=int, default=37322725)
    args = ap.parse_args()
    M = blz.Matrix.synth(args.rows, args.cols, args.nnz, 0x474C3764, P61)
    print(f"matrix {M.nrows} x {M.ncols}, {M.nnz} entries (GL7d19-shape synthetic), p = 2^61 - 1, left kernel; "
          f"medians of {ROUNDS} alternated rounds")
    for n in (8, 16):
        with blz.Context(P61, n) as ctx:
            ctx.set_matrix(M)
            rows = ctx.rows(blz.V)
            mb = rows * n * 8 / 1e6
            host = blz.rng_fill(rows * n, P61)
            dev = torch.from_numpy(host.view(np.int64).reshape(rows, n)).to("cuda:0")
            out = torch.empty_like(dev)
            ctx.set_block_device(blz.V, dev)            # the numbering goes up once
            ctx.get_block_device(blz.V, out=out)
            assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(-1), host), "device round trip"
            hp, dp = [], []
            for _ in range(ROUNDS):
                hp.append(wall(lambda: (ctx.set_block(blz.V, host), ctx.get_block(blz.V))))
                dp.append(wall(lambda: (ctx.set_block_device(blz.V, dev), ctx.get_block_device(blz.V, out=out))))
            h, d = statistics.median(hp), statistics.median(dp)
            imp = events(lambda: ctx.set_block_device(blz.V, dev))
            exp = events(lambda: ctx.get_block_device(blz.V, out=out))
            print(f"n = {n:2d}  block {rows} x {n} = {mb:.1f} MB")
            print(f"  (a) set + get of V   host path {h:9.2f} ms   device path {d:7.3f} ms (wall, two calls, synchronised)   "
                  f"host / device = {h / d:.0f}")
            for tag, ms in (("import", imp), ("export", exp)):
                rate = 2 * mb * 1e6 / (ms * 1e-3)
                print(f"      {tag} alone {ms * 1e3:7.1f} us: {2 * mb:.0f} MB moved, {rate / 1e12:.2f} TB/s = "
                      f"{100 * rate / CEILING:.0f} % of the {CEILING / 1e12:.1f} TB/s streaming ceiling")
            # (b): product not right reads V-side rows, writes TMP-side rows -- blz_time_kernel(0) is that product alone
            t = not ctx.right
            xr, yr = ctx.apply_rows(t)
            x = torch.from_numpy(blz.rng_fill(xr * n, P61).view(np.int64).reshape(xr, n)).to("cuda:0")
            y = torch.empty((yr, n), dtype=torch.int64, device="cuda:0")
            ctx.apply(t, x, out=y)
            ap_, pr = [], []
            for _ in range(ROUNDS):
                ap_.append(events(lambda: ctx.apply(t, x, out=y), reps=3))
                pr.append(ctx.time_kernel(0, 3))
            a, k = statistics.median(ap_), statistics.median(pr)
            print(f"  (b) apply {a * 1e3:7.1f} us   product alone (blz_time_kernel) {k * 1e3:7.1f} us   "
                  f"the two passes {1e3 * (a - k):6.1f} us = {100 * (a - k) / a:.0f} % of apply, {100 * (a - k) / k:.0f} % on top of the product")
            other = events(lambda: ctx.apply(not t, y, out=x), reps=5)
            print(f"      the other product through apply {other * 1e3:7.1f} us   (product alone {ctx.time_kernel(1, 3) * 1e3:7.1f} us)")
            ctx.apply_release()


if __name__ == "__main__":
    main()
