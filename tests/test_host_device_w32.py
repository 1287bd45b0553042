"""32-bit device blocks, the part that needs no GPU: the header declares the eight entry points and the library exports them,
`import blz` still does not pull torch in, blz.device_block32 reads a block off anything that looks like a tensor (run here
on fakes), blz.device_block is what it was, and the case list of tests/test_gpu_device_w32.py (tests/device_w32_ref.py)
reaches every form of every kernel of csrc/blz_devw32.hip.
"""
import os
import re
import subprocess
import sys

import pytest

import blz
import device_w32_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYDIR = os.path.join(ROOT, "block-lanczos-algorithm-parallelization_amd", "python")

EIGHT = {
    "blz_set_block_device32": "int blz_set_block_device32(blz_ctx *, int block, const uint32_t *dev, int64_t ld, void *stream, int64_t *bad);",
    "blz_get_block_device32": "int blz_get_block_device32(blz_ctx *, int block, uint32_t *dev, int64_t ld, void *stream);",
    "blz_apply_device32": "int blz_apply_device32(blz_ctx *, int transpose, const uint32_t *x, int64_t ldx, uint32_t *y, int64_t ldy, void *stream);",
    "blz_apply_pair_device32": "int blz_apply_pair_device32(blz_ctx *, int transpose_first, const uint32_t *x, int64_t ldx, uint32_t *y, "
                               "int64_t ldy, uint32_t *z, int64_t ldz, void *stream);",
    "blz_dot_device32": "int blz_dot_device32(blz_ctx *, int64_t rows, const uint32_t *x, int64_t ldx, const uint32_t *y, int64_t ldy, "
                        "uint64_t *c, void *stream);",
    "blz_dot_pair_device32": "int blz_dot_pair_device32(blz_ctx *, int64_t rows, const uint32_t *x0, int64_t ldx0, const uint32_t *x1, "
                             "int64_t ldx1, const uint32_t *y, int64_t ldy, uint64_t *c, void *stream);",
    "blz_combine_device32": "int blz_combine_device32(blz_ctx *, int64_t rows, int nterms, const uint32_t *const *x, const int64_t *ldx, "
                            "const uint64_t *const *a, uint32_t *z, int64_t ldz, void *stream);",
    "blz_combine_pair_device32": "int blz_combine_pair_device32(blz_ctx *, int64_t rows, int nterms, const uint32_t *const *x, "
                                 "const int64_t *ldx, const uint64_t *const *a0, const uint64_t *const *a1, uint32_t *z0, int64_t ldz0, "
                                 "uint32_t *z1, int64_t ldz1, void *stream);",
}
METHODS = ("set_block_device32", "get_block_device32", "apply32", "apply_pair32", "dot32", "dot_pair32", "combine32", "combine_pair32")


def squeeze(decl):
    return re.sub(r"\s+", "", decl.replace("blz_ctx *ctx", "blz_ctx *"))


def test_the_header_declares_the_eight_functions_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "blz.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, want in EIGHT.items():
        m = re.search(r"\bint\s+" + name + r"\s*\([^;]*;", hdr)
        assert m, name
        assert squeeze(m.group(0)) == squeeze(want), (m.group(0), want)
        assert hasattr(blz.lib(), name), name
    for meth in METHODS:
        assert callable(getattr(blz.Context, meth)), meth
    for absent in ("blz_rref_device32", "blz_take_local_device32", "blz_put_local_device32"):      # stated limits, not built
        assert not re.search(r"\b" + absent + r"\s*\(", hdr) and not hasattr(blz.lib(), absent)


def test_import_blz_leaves_torch_out():
    code = ("import sys; sys.path.insert(0, %r); import blz; blz.lib(); "
            "assert 'torch' not in sys.modules, 'import blz pulled torch in'; "
            "assert callable(blz.device_block32) and callable(blz.Context.dot32); print('clean')" % PYDIR)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stderr


# ------------------------------------------------------------------------------------------------ fake tensors


class Dev:
    def __init__(self, type_, index):
        self.type, self.index = type_, index

    def __str__(self):
        return self.type if self.index is None else f"{self.type}:{self.index}"


class Fake:
    """what device_block32 looks at, and nothing else"""

    def __init__(self, shape, stride, dtype="torch.uint32", device=("cuda", 0), ptr=0x7F0000001000):
        self.shape, self._stride, self.dtype, self.device, self._ptr = tuple(shape), tuple(stride), dtype, Dev(*device), ptr

    def stride(self):
        return self._stride

    def data_ptr(self):
        return self._ptr


@pytest.mark.parametrize("dtype", ("torch.uint32", "torch.int32"))
def test_both_layouts_and_both_dtypes_are_accepted(dtype):
    assert blz.DEVICE_DTYPES32 == ("torch.uint32", "torch.int32")
    assert blz.device_block32(Fake((40, 8), (8, 1), dtype), 8, 40, 0) == (0x7F0000001000, 40, 8, 0)
    assert blz.device_block32(Fake((40, 8), (11, 1), dtype, ptr=4100), 8, 40, 0) == (4100, 40, 11, 0)    # ld = n + 3, 4-byte base
    assert blz.device_block32(Fake((320,), (1,), dtype), 8, 40, 0) == (0x7F0000001000, 40, 8, 0)         # flat
    assert blz.device_block32(Fake((40, 8), (8, 1), dtype, device=("cuda", 3)), 8)[1:] == (40, 8, 3)
    assert blz.device_block32(Fake((30, 1), (4, 7), dtype), 1, 30, 0)[1:3] == (30, 4)
    assert blz.device_block32(Fake((1, 8), (1, 1), dtype), 8, 1, 0)[1:3] == (1, 8)


@pytest.mark.parametrize("fake, n, rows, why", [
    (Fake((40, 8), (8, 1), "torch.int64"), 8, 40, "dtype"),
    (Fake((40, 8), (8, 1), "torch.uint64"), 8, 40, "dtype"),
    (Fake((40, 8), (8, 1), "torch.float64"), 8, 40, "dtype"),
    (Fake((40, 8), (8, 1), "torch.float32"), 8, 40, "dtype"),
    (Fake((40, 8), (16, 2)), 8, 40, "inner stride"),
    (Fake((40, 8), (1, 40)), 8, 40, "inner stride"),
    (Fake((40, 8), (7, 1)), 8, 40, "ld = 7"),
    (Fake((39, 8), (8, 1)), 8, 40, "39 rows"),
    (Fake((321,), (1,)), 8, 40, "whole number of rows"),
    (Fake((320,), (2,)), 8, 40, "contiguous"),
    (Fake((40, 4), (4, 1)), 8, 40, "columns"),
    (Fake((5, 8, 8), (64, 8, 1)), 8, 40, "dimensions"),
    (Fake((40, 8), (8, 1), device=("cpu", None)), 8, 40, "not on a GPU"),
    (Fake((40, 8), (8, 1), device=("cuda", 1)), 8, 40, "device 1"),
])
def test_what_the_helper_refuses(fake, n, rows, why):
    with pytest.raises(ValueError) as e:
        blz.device_block32(fake, n, rows, 0)
    assert why in str(e.value), str(e.value)


def test_the_64_bit_helper_is_what_it_was():
    assert blz.DEVICE_DTYPES == ("torch.uint64", "torch.int64")
    for dtype in ("torch.int32", "torch.uint32"):
        with pytest.raises(ValueError) as e:
            blz.device_block(Fake((40, 8), (8, 1), dtype), 8, 40, 0)
        assert "dtype" in str(e.value) and "torch.uint64, torch.int64" in str(e.value)
    assert blz.device_block(Fake((40, 8), (11, 1), "torch.int64", ptr=4096), 8, 40, 0) == (4096, 40, 11, 0)
    with pytest.raises(ValueError) as e:                # the term helpers still go through it by default
        blz.device_terms([(Fake((40, 8), (8, 1), "torch.int32"), Fake((8, 8), (8, 1), "torch.uint64"))], 8, 0)
    assert "dtype" in str(e.value)
    rows, args = blz.device_terms([(Fake((40, 8), (8, 1), "torch.int32"), Fake((8, 8), (8, 1), "torch.uint64"))], 8, 0,
                                  blz.device_block32)
    assert rows == 40 and len(args) == 1


# ------------------------------------------------------------------------------------------------ the launcher's choices


def test_the_width_of_a_lane_access():
    assert ref.width(0, 8, 8) == 4 and ref.width(0, 12, 8) == 4 and ref.width(0, 64, 64) == 4
    assert ref.width(8, 8, 8) == 2 and ref.width(0, 10, 8) == 2 and ref.width(0, 6, 6) == 2 and ref.width(0, 2, 2) == 2
    assert ref.width(4, 8, 8) == 1 and ref.width(12, 8, 8) == 1 and ref.width(0, 9, 8) == 1 and ref.width(0, 5, 5) == 1
    assert ref.width(0, 1, 1) == 1 and ref.width(0, 4, 1) == 1 and ref.width(0, 20, 17) == 1
    # a vector access never reaches the words n .. ld-1: the width divides n
    for n in range(1, 65):
        for ld in range(n, n + 9):
            for a in (0, 4, 8, 12):
                w = ref.width(a, ld, n)
                assert n % w == 0 and ld % w == 0 and a % (4 * w) == 0
    assert [ref.tile_rows(n) for n in (1, 2, 3, 8, 16, 17, 33, 64)] == [2048, 1024, 512, 256, 128, 64, 32, 32]
    assert [ref.thread_tile(n) for n in (1, 2, 16, 17, 64)] == [1, 2, 2, 4, 4]
    assert [ref.dot_slices(n) for n in (1, 2, 8, 16, 32, 64)] == [256, 256, 16, 4, 4, 1]
    # four terms at n = 64: 64 KB, two workgroups of 1024 threads on a CU; the pair: 128 KB, one
    assert ref.combine_shape(64, 4, 1) == (65536, 1024, 2) and ref.combine_shape(64, 4, 2) == (131072, 1024, 1)
    assert ref.combine_shape(64, 2, 1)[1:] == (256, 8) and ref.combine_shape(16, 4, 2)[1:] == (256, 8)


def test_the_gpu_case_list_reaches_every_form_of_every_kernel():
    assert ref.dot_forms_reached(pair=False) == ref.ALL_DOT_FORMS
    assert ref.dot_forms_reached(pair=True) == ref.ALL_DOT_FORMS
    assert ref.combine_forms_reached(1) == ref.ALL_VECTOR_FORMS
    assert ref.combine_forms_reached(2) == ref.ALL_VECTOR_FORMS
    assert ref.io_forms_reached() == ref.ALL_VECTOR_FORMS
    # the pointers 4, 8 and 12 bytes past a 16-byte boundary are all in the list
    assert {off for _, off, _, _ in ref.DOT_LAYOUTS} == {0, 1, 2, 3}
    assert {px for px, _, _, _ in ref.DOT_LAYOUTS} == {0, 1, 2, 3, 4}
    for n in ref.WIDTHS:                                # one short of the kernel's tile, the tile, one past; two tiles a workgroup
        small, big = ref.dot_rows(n)
        tr = ref.tile_rows(n)
        assert {tr - 1, tr, tr + 1} <= set(small)
        cap = ref.dot_max_blocks(n, 256)
        assert big > 2 * cap * tr and big % tr != 0
