"""bench.py on one GPU as it is run for every change: a plain run (set-up, warm-up, exactly --steps timed steps, the line)
and --dump-outputs, whose files must hold what the timed path computed -- the same words as the CPU oracle after as many
iterations, and the same files from one run to the next.  --full must still carry the diagnostics that moved behind it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench as bench_py
import blz
import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", *args],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def words(a):
    """bench.words_f64 undone: (high, low) float64 halves -> u64 words"""
    return (a[..., 0].astype(np.uint64) << np.uint64(32)) | a[..., 1].astype(np.uint64)


def test_plain_run_times_the_steps_asked_and_dumps_what_they_computed(tmp_path):
    steps, warmup = 3, 2
    d = bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == steps and d["warmup"] == warmup and d["value"] > 0 and d["ms_per_step"] > 0
    assert len(d["repeats"]["ms_per_step"]) == 1                  # one timed region of exactly --steps steps
    assert not {"roofline", "kernels", "cpu_baseline", "cpu_reference", "extra"} & set(d), sorted(d)

    got = load(tmp_path / "a")
    assert set(got) == {"v", "p", "v_rows", "p_rows", "vtAv", "vtAAv", "winv", "d", "iterations"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in got) <= 64 << 20
    assert int(got["iterations"][0]) == warmup + steps

    # the same words as the oracle after warm-up + timed steps (tiny: every row of each block is in the sample)
    w = bench_py.WORKLOADS["tiny"]
    M = blz.Matrix.synth(w["rows"], w["cols"], w["nnz"], w["seed"], w["prime"], pattern=w["pattern"])
    recs = []
    want = orc.block_lanczos(orc.Matrix(M.nrows, M.ncols, M.i, M.j, M.x), w["n"], w["prime"], right=w["right"],
                             stop_after=warmup + steps, trace=recs.append)
    assert len(recs) == want["iterations"] == warmup + steps
    for name in ("v", "p"):
        rows = got[name + "_rows"].astype(np.int64)
        assert np.array_equal(rows, np.arange(want[name].size // w["n"])), name
        assert np.array_equal(words(got[name]), want[name].reshape(-1, w["n"])[rows]), name
    for name in ("vtAv", "vtAAv", "winv", "d"):               # the n x n operands of the last step
        assert np.array_equal(words(got[name]).ravel(), recs[-1][name]), name

    # same arguments, same inputs, same files
    bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "b"))
    again = load(tmp_path / "b")
    assert set(again) == set(got) and all(np.array_equal(again[k], got[k]) for k in got)


def test_full_run_keeps_the_diagnostics():
    d = bench("--steps", "3", "--warmup", "1", "--full", "--ref-iterations", "0")
    assert len(d["repeats"]["ms_per_step"]) == 5
    assert d["roofline"]["achieved"] > 0 and d["kernels"]["spmv1"]["launches"] > 0
    assert d["cpu_baseline"]["gpu_equals_cpu_after_sample"] is True
