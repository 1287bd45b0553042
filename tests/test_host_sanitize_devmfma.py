"""The dispatch decision and the image layout of the device block algebra on the matrix cores (csrc/blz_devmfma_plan.h, plain C)
compiled with AddressSanitizer + UndefinedBehaviorSanitizer into the stand-alone program tests/host_sanitize_devmfma.c and run
over the whole domain of the decision.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_dispatch_and_image_layout_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_sanitize_devmfma")
    cc = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
          "-fno-omit-frame-pointer", "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "host_sanitize_devmfma.c"),
          "-o", exe]
    build = subprocess.run(cc, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "clean under ASan + UBSan" in run.stdout
