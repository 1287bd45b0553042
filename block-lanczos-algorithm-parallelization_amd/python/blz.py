"""ctypes binding of libblz_hip.so (include/blz.h) for tests and bench.py.

Host-language note: the reference is a C program, so the product's host side is C
(csrc/host/lanczos_modp.c drives the same ABI).  This module is only the thin Python view the
test-suite and the benchmark use; it adds no computation of its own and there is NO fallback:
if the library is missing, or no GPU is visible, calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG, "lib", "libblz_hip.so")

V, TMP, AV, P = 0, 1, 2, 3
VTAV, VTAAV, WINV, D = 0, 1, 2, 3
OK, EINVAL, EIO, EFORMAT, ENOMEM, EHIP, ENOGPU, ECOMM = 0, -1, -2, -3, -4, -5, -6, -7

U64P = C.POINTER(C.c_uint64)
_lib = None


class BlzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"blz error {code}: {msg}")
        self.code = code


class Coo(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64),
                ("i", C.POINTER(C.c_int32)), ("j", C.POINTER(C.c_int32)), ("x", C.POINTER(C.c_uint32))]


class Csr(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int64), ("nnz", C.c_int64),
                ("row_ptr", C.POINTER(C.c_uint32)), ("col_idx", C.POINTER(C.c_int32)),
                ("val", C.POINTER(C.c_uint32))]


class PlanLaunch(C.Structure):
    """blz_plan_launch of include/blz.h."""
    _fields_ = [(k, C.c_int32) for k in ("form", "xcd_ranges", "split_log2", "st_gathers")] + \
               [(k, C.c_int64) for k in ("grid_stream", "grid_heavy", "grid_combine", "grid_medium")]


class Plan(C.Structure):
    """blz_plan of include/blz.h."""
    _fields_ = [(k, C.c_int64) for k in ("rows", "cols", "nnz")] + \
               [(k, C.c_int32) for k in ("pieces", "width", "chunk", "num_cu", "max_dot_blocks", "tail_batch", "xcd_ranges")] + \
               [("heavy_thr", C.c_uint32)] + \
               [(k, C.c_int32) for k in ("n_medium", "n_heavy", "n_multi", "st_ok", "st_tr", "st_pair", "st_dyn", "st_deep",
                                         "st_interleave", "st_capw", "st_per_cu", "panel_rows", "packed", "dot_supported",
                                         "fused", "fuse_local_off", "short_side")] + \
               [("locality", C.c_double), ("plain", PlanLaunch), ("dot", PlanLaunch)]


FORMS = ("spmv", "staged", "panel")


class DevalgPlan(C.Structure):
    """struct blz_devalg_plan of include/blz.h."""
    _fields_ = [(k, C.c_int32) for k in ("form", "tile_rows", "wavefronts", "fold_tiles")] + \
               [(k, C.c_int64) for k in ("min_rows", "lds_bytes")]


DEVOP_DOT, DEVOP_DOT_PAIR, DEVOP_COMBINE, DEVOP_COMBINE_PAIR = range(4)     # BLZ_DEVOP_* of include/blz.h


def lib():
    """Load libblz_hip.so.  Raises if it has not been built: there is no Python/CPU substitute."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built (run __graft_entry__.build() or make in {PKG})")
        # the pool's host driver only supports dmabuf IPC; RCCL across processes needs this before HIP initialises
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L.blz_last_error.restype = C.c_char_p
        L.blz_rng_next.restype = C.c_uint64
        L.blz_rows.restype = C.c_int64
        L.blz_local_rows.restype = C.c_int64
        L.blz_iterations.restype = C.c_int64
        L.blz_local_nnz.restype = C.c_int64
        L.blz_matrix_stream_bytes.restype = C.c_int64
        L.blz_panel_rows.restype = C.c_int64
        L.blz_prepare_key.restype = C.c_uint64
        L.blz_file_hash.restype = C.c_uint64
        L.blz_prepared_free.restype = None
        L.blz_prepared_free.argtypes = [C.c_void_p]
        L.blz_destroy.restype = None
        L.blz_coo_free.restype = None
        L.blz_csr_free.restype = None
        L.blz_values_free.restype = None
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise BlzError(rc, lib().blz_last_error().decode(errors="replace"))


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(U64P) if a is not None else None


def device_count():
    return int(lib().blz_device_count())


DEVICE_DTYPES = ("torch.uint64", "torch.int64")     # the same 64 bits either way: no conversion


def device_block(t, n, rows=None, device=None):
    """(pointer, rows, ld, device index) of a block held by a torch tensor -- or by any object with data_ptr(), shape,
    stride(), dtype and device, which is all this looks at: torch is not imported here.  Two layouts: 2-D (rows, n) with
    strides (ld, 1), ld >= n, or 1-D contiguous with rows * n elements.  rows / device, when given, are what the caller
    expects (the block's row count, the context's device index).  Anything else is a ValueError that names the fault."""
    return _device_block(t, n, rows, device, DEVICE_DTYPES)


DEVICE_DTYPES32 = ("torch.uint32", "torch.int32")   # the same 32 bits either way: a residue >= 2**31 is not negative


def device_block32(t, n, rows=None, device=None):
    """device_block() for a block of 32-bit words (the ...32 methods of Context, p < 2**32): the same two layouts and the same
    faults, the dtype one of DEVICE_DTYPES32 and ld counted in 32-bit words."""
    return _device_block(t, n, rows, device, DEVICE_DTYPES32)


def _device_block(t, n, rows, device, dtypes):
    """what device_block() and device_block32() share: everything but the dtypes they accept"""
    if str(t.dtype) not in dtypes:
        raise ValueError(f"device block: dtype {t.dtype} is not one of {', '.join(dtypes)}")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"device block: the tensor lives on {t.device}, not on a GPU")
    index = t.device.index if t.device.index is not None else 0
    if device is not None and index != device:
        raise ValueError(f"device block: the tensor lives on device {index}, the context on device {device}")
    shape, stride = tuple(t.shape), tuple(t.stride())
    if len(shape) == 2:
        if shape[1] != n:
            raise ValueError(f"device block: {shape[1]} columns, the block width is {n}")
        if n > 1 and stride[1] != 1 and shape[0] > 0:   # (a block of no rows has no words: torch may say any stride)
            raise ValueError(f"device block: inner stride {stride[1]}, rows must be contiguous")
        got, ld = shape[0], (stride[0] if shape[0] > 1 else max(stride[0], n))
        if ld < n:
            raise ValueError(f"device block: row stride ld = {ld} is less than n = {n}")
    elif len(shape) == 1:
        if stride[0] != 1 and shape[0] > 1:
            raise ValueError(f"device block: a 1-D block must be contiguous (stride {stride[0]})")
        if shape[0] % n:
            raise ValueError(f"device block: {shape[0]} elements are not a whole number of rows of {n}")
        got, ld = shape[0] // n, n
    else:
        raise ValueError(f"device block: {len(shape)} dimensions; a block is (rows, n) or flat")
    if rows is not None and got != rows:
        raise ValueError(f"device block: {got} rows, the block has {rows}")
    return int(t.data_ptr()), int(got), int(ld), int(index)


MAX_TERMS = 4       # BLZ_MAX_TERMS of include/blz.h


def device_square(t, n, device=None):
    """pointer of an n x n operand of the block algebra (a coefficient matrix, the result of dot) held by a tensor -- or by
    anything with data_ptr(), shape, stride(), dtype and device: (n, n), contiguous, uint64 or int64, on the context's device.
    Anything else is a ValueError that names the fault.  torch is not imported here."""
    if str(t.dtype) not in DEVICE_DTYPES:
        raise ValueError(f"n x n operand: dtype {t.dtype} is not one of {', '.join(DEVICE_DTYPES)}")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"n x n operand: the tensor lives on {t.device}, not on a GPU")
    index = t.device.index if t.device.index is not None else 0
    if device is not None and index != device:
        raise ValueError(f"n x n operand: the tensor lives on device {index}, the context on device {device}")
    shape, stride = tuple(t.shape), tuple(t.stride())
    if shape != (n, n):
        raise ValueError(f"n x n operand: shape {shape}, not ({n}, {n})")
    if n > 1 and stride != (n, 1):
        raise ValueError(f"n x n operand: strides {stride}, the operand must be contiguous")
    return int(t.data_ptr())


COEF_PANELS = 5     # BLZ_COEF_PANELS of include/blz.h, and the panel indices of its enum
COEF_V_AV, COEF_V_V, COEF_V_P, COEF_P_P, COEF_P_V = 0, 1, 2, 3, 4


def device_words(t, shape, dtypes=DEVICE_DTYPES, device=None, what="operand"):
    """pointer of a contiguous operand of the small algebra that is not a block: `shape` words of one of `dtypes` on the
    context's device -- the (5, n, n) coefficient panels, d (n,), npiv (1,), info (n + 1,) of int64.  Looks at data_ptr(),
    shape, stride(), dtype and device only; anything else is a ValueError that names the fault.  torch is not imported here."""
    shape = tuple(shape)
    if str(t.dtype) not in dtypes:
        raise ValueError(f"{what}: dtype {t.dtype} is not one of {', '.join(dtypes)}")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"{what}: the tensor lives on {t.device}, not on a GPU")
    index = t.device.index if t.device.index is not None else 0
    if device is not None and index != device:
        raise ValueError(f"{what}: the tensor lives on device {index}, the context on device {device}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: shape {tuple(t.shape)}, not {shape}")
    want, run = [], 1
    for extent in reversed(shape):
        want.insert(0, run)
        run *= extent
    if any(s != w for s, w, extent in zip(tuple(t.stride()), want, shape) if extent > 1):
        raise ValueError(f"{what}: strides {tuple(t.stride())}, the operand must be contiguous")
    return int(t.data_ptr())


def device_coef(t, n, device=None):
    """pointer of the (COEF_PANELS, n, n) contiguous coefficient panels of Context.ortho_coeffs"""
    return device_words(t, (COEF_PANELS, n, n), DEVICE_DTYPES, device, "coefficient panels")


def device_info(t, n, device=None):
    """pointer of the (n + 1,) int64 words [rank, pivots] of Context.rref"""
    return device_words(t, (n + 1,), ("torch.int64",), device, "info")


def device_terms(terms, n, device=None, block=None):
    """(rows, [(pointer of X, ld of X, pointer of A), ...]) of the 1..MAX_TERMS pairs (X, A) of Context.combine: every X goes
    through device_block, every A through device_square; the rows are the first block's and all blocks must agree."""
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"combine: {len(terms)} terms, not 1..{MAX_TERMS}")
    rows, out = None, []
    for k, pair in enumerate(terms):
        if len(pair) != 2:
            raise ValueError(f"combine: term {k} is not a pair (X, A)")
        try:
            px, rows, ldx, _ = (block or device_block)(pair[0], n, rows, device)
            pa = device_square(pair[1], n, device)
        except ValueError as e:
            raise ValueError(f"combine: term {k}: {e}") from None
        out.append((px, ldx, pa))
    return rows, out


def device_pair(t, n, device=None):
    """pointer of the (2, n, n) contiguous panels of Context.dot_pair: [0] = x0^T y, [1] = x1^T y"""
    return device_words(t, (2, n, n), DEVICE_DTYPES, device, "inner product pair")


def device_pair_terms(terms, n, device=None, block=None):
    """(rows, [(pointer of X, ld of X, pointer of A0 or None, pointer of A1 or None), ...]) of the 1..MAX_TERMS triples
    (X, A0, A1) of Context.combine_pair: every X goes through device_block, every coefficient that is not None through
    device_square; all blocks agree in their rows, every term enters an output and every output has a term."""
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError(f"combine_pair: {len(terms)} terms, not 1..{MAX_TERMS}")
    rows, out = None, []
    for k, triple in enumerate(terms):
        if len(triple) != 3:
            raise ValueError(f"combine_pair: term {k} is not a triple (X, A0, A1)")
        if triple[1] is None and triple[2] is None:
            raise ValueError(f"combine_pair: term {k} enters neither output (A0 and A1 are both None)")
        try:
            px, rows, ldx, _ = (block or device_block)(triple[0], n, rows, device)
            pa = [None if a is None else device_square(a, n, device) for a in triple[1:]]
        except ValueError as e:
            raise ValueError(f"combine_pair: term {k}: {e}") from None
        out.append((px, ldx, pa[0], pa[1]))
    for o in (0, 1):
        if all(term[2 + o] is None for term in out):
            raise ValueError(f"combine_pair: output z{o} has no term (every A{o} is None)")
    return rows, out


def device_pair_out(out, n, rows, device=None, block=None):
    """[(pointer, ld), (pointer, ld)] of the two outputs (z0, z1) of Context.combine_pair: blocks of `rows` rows each"""
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("combine_pair: out is not a pair (z0, z1)")
    res = []
    for o, z in enumerate(out):
        try:
            pz, _, ldz, _ = (block or device_block)(z, n, rows, device)
        except ValueError as e:
            raise ValueError(f"combine_pair: output z{o}: {e}") from None
        res.append((pz, ldz))
    return res


TRIPLET_INDEX_DTYPES = {"torch.int32": 4, "torch.int64": 8}
TRIPLET_VALUE_DTYPES = {"torch.uint32": 4, "torch.int32": 4, "torch.uint64": 8, "torch.int64": 8}   # bits read as unsigned


def _device_vector(t, what, dtypes, device, length=None):
    """(pointer, element bytes, length) of a 1-D contiguous tensor of one of `dtypes` on the context's device"""
    if str(t.dtype) not in dtypes:
        raise ValueError(f"device triplets: {what}: dtype {t.dtype} is not one of {', '.join(dtypes)}")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"device triplets: {what} lives on {t.device}, not on a GPU")
    index = t.device.index if t.device.index is not None else 0
    if device is not None and index != device:
        raise ValueError(f"device triplets: {what} lives on device {index}, the context on device {device}")
    shape, stride = tuple(t.shape), tuple(t.stride())
    if len(shape) != 1:
        raise ValueError(f"device triplets: {what} has {len(shape)} dimensions, not 1")
    if shape[0] > 1 and stride[0] != 1:
        raise ValueError(f"device triplets: {what} must be contiguous (stride {stride[0]})")
    if length is not None and shape[0] != length:
        raise ValueError(f"device triplets: {what} has {shape[0]} elements, i has {length}")
    return int(t.data_ptr()), dtypes[str(t.dtype)], int(shape[0])


def device_triplets(i, j, x=None, device=None):
    """(pointer of i, pointer of j, idx_bytes, pointer of x or None, val_bytes, nnz) of the triplets of
    Context.set_matrix_device held by torch tensors -- or by anything with data_ptr(), shape, stride(), dtype and device: i
    and j 1-D contiguous of ONE dtype, int32 or int64 (a row of a (2, nnz) index tensor is such a vector), x None or 1-D
    contiguous of TRIPLET_VALUE_DTYPES with as many elements.  Anything else is a ValueError that names the fault.  torch is
    not imported here."""
    pi, ib, nnz = _device_vector(i, "i", TRIPLET_INDEX_DTYPES, device)
    pj, jb, _ = _device_vector(j, "j", TRIPLET_INDEX_DTYPES, device, nnz)
    if ib != jb:
        raise ValueError(f"device triplets: i is {i.dtype} and j is {j.dtype}; the two must agree")
    if x is None:
        return pi, pj, ib, None, 0, nnz
    px, vb, _ = _device_vector(x, "x", TRIPLET_VALUE_DTYPES, device, nnz)
    return pi, pj, ib, px, vb, nnz


def device_rhs(t, n, rows=None, device=None):
    """(pointer, rows, k, ld) of the right-hand sides of Context.set_rhs_device -- or of the x of Context.solution_device --
    held by a torch tensor, or by anything with data_ptr(), shape, stride(), dtype and device: (rows,) for one right-hand
    side or (rows, k) for k of them, 1 <= k <= min(n, MAX_RHS), the last dimension contiguous, the row stride ld >= k taken
    from the tensor, one of DEVICE_DTYPES, on the context's device.  Anything else is a ValueError that names the fault.
    torch is not imported here."""
    return _device_rhs(t, n, rows, device, DEVICE_DTYPES)


def device_rhs32(t, n, rows=None, device=None):
    """device_rhs() for 32-bit words (the ...32 methods of Context, p < 2**32): the dtype one of DEVICE_DTYPES32 and ld
    counted in 32-bit words."""
    return _device_rhs(t, n, rows, device, DEVICE_DTYPES32)


def _device_rhs(t, n, rows, device, dtypes):
    if str(t.dtype) not in dtypes:
        raise ValueError(f"device right-hand side: dtype {t.dtype} is not one of {', '.join(dtypes)}")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"device right-hand side: the tensor lives on {t.device}, not on a GPU")
    index = t.device.index if t.device.index is not None else 0
    if device is not None and index != device:
        raise ValueError(f"device right-hand side: the tensor lives on device {index}, the context on device {device}")
    shape, stride = tuple(t.shape), tuple(t.stride())
    if len(shape) == 1:
        got, k, ld = shape[0], 1, (stride[0] if shape[0] > 1 else max(stride[0], 1))
    elif len(shape) == 2:
        got, k = shape
        if k > 1 and stride[1] != 1 and got > 0:
            raise ValueError(f"device right-hand side: inner stride {stride[1]}, the last dimension must be contiguous")
        ld = stride[0] if got > 1 else max(stride[0], k)
    else:
        raise ValueError(f"device right-hand side: {len(shape)} dimensions; it is (rows,) or (rows, k)")
    if not 1 <= k <= min(n, MAX_RHS):
        raise ValueError(f"device right-hand side: k = {k} right-hand sides: between 1 and min(n = {n}, {MAX_RHS}) are possible")
    if ld < k:
        raise ValueError(f"device right-hand side: row stride ld = {ld} is less than k = {k}")
    if rows is not None and got != rows:
        raise ValueError(f"device right-hand side: {got} rows, not {rows}")
    return int(t.data_ptr()), int(got), int(k), int(ld)


class Matrix:
    """struct sparsematrix_t of the reference (sequential/lanczos_modp.c:55-62) as numpy arrays."""

    def __init__(self, nrows, ncols, i, j, x, x_hi=None):
        """x_hi (wide value mode): the high limbs of the entries, parallel to x -- entry k is x[k] + 2**32 * x_hi[k]."""
        self.x_hi = None if x_hi is None else np.ascontiguousarray(x_hi, dtype=np.uint32)
        assert self.x_hi is None or self.x_hi.shape == (len(i),)
        self.i = np.ascontiguousarray(i, dtype=np.int32)
        self.j = np.ascontiguousarray(j, dtype=np.int32)
        self.x = np.ascontiguousarray(x, dtype=np.uint32)
        self.nrows, self.ncols, self.nnz = int(nrows), int(ncols), len(self.i)
        self.c = Coo(self.nrows, self.ncols, self.nnz, self.i.ctypes.data_as(C.POINTER(C.c_int32)),
                     self.j.ctypes.data_as(C.POINTER(C.c_int32)), self.x.ctypes.data_as(C.POINTER(C.c_uint32)))

    @staticmethod
    def _take(M):
        n = int(M.nnz)
        out = Matrix(M.nrows, M.ncols, np.ctypeslib.as_array(M.i, (max(n, 1),))[:n].copy(),
                     np.ctypeslib.as_array(M.j, (max(n, 1),))[:n].copy(),
                     np.ctypeslib.as_array(M.x, (max(n, 1),))[:n].copy())
        lib().blz_coo_free(C.byref(M))
        return out

    @staticmethod
    def load(path, prime):
        """sparsematrix_mm_load(), sequential/lanczos_modp.c:199-263."""
        M = Coo()
        check(lib().blz_mm_load(path.encode(), C.c_uint64(prime), C.byref(M)))
        return Matrix._take(M)

    @staticmethod
    def load_signed(path):
        """blz_mm_load_signed(): x holds the int32 bit pattern of every entry (signed value mode; no prime)."""
        M = Coo()
        check(lib().blz_mm_load_signed(path.encode(), C.byref(M)))
        return Matrix._take(M)

    @staticmethod
    def load_wide(path, prime):
        """blz_mm_load_wide(): every entry an int64 read as its residue mod prime; x holds the low limbs and x_hi the high
        ones (None when no residue reaches 2**32)."""
        M = Coo()
        hi = C.POINTER(C.c_uint32)()
        check(lib().blz_mm_load_wide(path.encode(), C.c_uint64(prime), C.byref(M), C.byref(hi)))
        n = int(M.nnz)
        x_hi = np.ctypeslib.as_array(hi, (max(n, 1),))[:n].copy() if hi else None
        lib().blz_values_free(hi)
        out = Matrix._take(M)
        if x_hi is not None:
            out.x_hi = x_hi
        return out

    def residues(self):
        """the entries as Python-sized integers in an int64 array (x + 2**32 * x_hi)"""
        r = self.x.astype(np.int64)
        return r if self.x_hi is None else r + (self.x_hi.astype(np.int64) << 32)

    @staticmethod
    def synth(nrows, ncols, nnz, seed, prime, pattern=False):
        M = Coo()
        check(lib().blz_synth_coo(C.c_int64(nrows), C.c_int64(ncols), C.c_int64(nnz), C.c_uint64(seed),
                                  C.c_int(int(pattern)), C.c_uint64(prime), C.byref(M)))
        return Matrix._take(M)

    @staticmethod
    def synth_part(nrows, ncols, nnz, seed, prime, rows=None, cols=None, pattern=False):
        """the entries of synth(...)'s matrix in rows [rows[0], rows[1]) and columns [cols[0], cols[1]), global indices,
        made without the rest of the matrix (blz_synth_coo_part)"""
        r0, r1 = rows if rows is not None else (0, nrows)
        c0, c1 = cols if cols is not None else (0, ncols)
        M = Coo()
        check(lib().blz_synth_coo_part(C.c_int64(nrows), C.c_int64(ncols), C.c_int64(nnz), C.c_uint64(seed), C.c_int(int(pattern)),
                                       C.c_uint64(prime), C.c_int64(r0), C.c_int64(r1), C.c_int64(c0), C.c_int64(c1), C.byref(M)))
        return Matrix._take(M)

    @staticmethod
    def synth_structured(nrows, ncols, nnz, seed, prime, pattern=False, hot_pct=40, band_pct=30, band=4096):
        """Heavy-tailed column degrees + banded supports (blz_synth_structured): the extra, non-headline workload."""
        M = Coo()
        check(lib().blz_synth_structured(C.c_int64(nrows), C.c_int64(ncols), C.c_int64(nnz), C.c_uint64(seed),
                                         C.c_int(int(pattern)), C.c_uint64(prime), C.c_int(hot_pct), C.c_int(band_pct),
                                         C.c_int64(band), C.byref(M)))
        return Matrix._take(M)

    def save(self, path):
        check(lib().blz_mm_save_coo(path.encode(), C.byref(self.c)))

    def csr(self, transpose=False, pattern=True):
        A = Csr()
        check(lib().blz_csr_from_coo(C.byref(self.c), C.c_int(int(transpose)), C.c_int(int(pattern)), C.byref(A)))
        rp = np.ctypeslib.as_array(A.row_ptr, (A.rows + 1,)).copy()
        ci = np.ctypeslib.as_array(A.col_idx, (max(A.nnz, 1),))[:A.nnz].copy()
        va = np.ctypeslib.as_array(A.val, (max(A.nnz, 1),))[:A.nnz].copy() if A.val else None
        bounds = lambda parts: _partition(A, parts)
        res = dict(rows=int(A.rows), cols=int(A.cols), nnz=int(A.nnz), row_ptr=rp, col_idx=ci, val=va)
        res["partition"] = {p: bounds(p) for p in (1, 2, 3, 4, 8)}
        lib().blz_csr_free(C.byref(A))
        return res


def _partition(A, parts):
    b = (C.c_int64 * (parts + 1))()
    check(lib().blz_partition_rows(C.byref(A), C.c_int(parts), b))
    return list(b)


def shard_matrix(M, right, rank, nranks, chunks=1):
    """blz_shard_matrix(): the slabs, bounds and strides rank `rank` of `nranks` works with (host only)."""
    slabs = (Csr * 2)()
    b0 = (C.c_int64 * (nranks + 1))()
    b1 = (C.c_int64 * (nranks + 1))()
    stride = (C.c_int64 * 2)()
    check(lib().blz_shard_matrix(C.byref(M.c), C.c_int(int(right)), C.c_int(rank), C.c_int(nranks), C.c_int(chunks), slabs,
                                 b0, b1, stride))
    out = []
    for A in slabs:
        rp = np.ctypeslib.as_array(A.row_ptr, (A.rows + 1,)).copy()
        ci = np.ctypeslib.as_array(A.col_idx, (max(A.nnz, 1),))[:A.nnz].copy()
        va = np.ctypeslib.as_array(A.val, (max(A.nnz, 1),))[:A.nnz].copy() if A.val else np.ones(A.nnz, np.uint32)
        out.append(dict(rows=int(A.rows), cols=int(A.cols), nnz=int(A.nnz), row_ptr=rp, col_idx=ci, val=va))
        lib().blz_csr_free(C.byref(A))
    return dict(slabs=out, bounds=[list(b0), list(b1)], stride=list(stride), chunks=chunks if nranks > 1 else 1)


class Prepared:
    """blz_prepared: the rank-independent part of a matrix's set-up (renumbering, CSR(M), CSR(M^T), partition), made once
    (prepare / prepare_for), shared by several contexts, saved to and mmapped from a cache file."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def prepare(M, right, nranks, chunks=1, reorder=1, rows_per_line=2, hot_cap=0, min_share=0.25):
        h = C.c_void_p()
        check(lib().blz_prepare(C.byref(M.c), C.c_int(int(right)), C.c_int(nranks), C.c_int(chunks), C.c_int(reorder),
                                C.c_int(rows_per_line), C.c_int64(hot_cap), C.c_double(min_share), C.byref(h)))
        return Prepared(h)

    @staticmethod
    def prepare_rank(row_part, col_part, nrows, ncols, nnz_total, right, rank, nranks, row_bounds, col_bounds, chunks=1):
        """one rank's prepared matrix from its own rows / columns of M alone (blz_prepare_rank)"""
        rb = np.ascontiguousarray(row_bounds, dtype=np.int64)
        cb = np.ascontiguousarray(col_bounds, dtype=np.int64)
        assert len(rb) == nranks + 1 and len(cb) == nranks + 1
        h = C.c_void_p()
        check(lib().blz_prepare_rank(C.byref(row_part.c), C.byref(col_part.c), C.c_int64(nrows), C.c_int64(ncols),
                                     C.c_int64(nnz_total), C.c_int(int(right)), C.c_int(rank), C.c_int(nranks), C.c_int(chunks),
                                     rb.ctypes.data_as(C.POINTER(C.c_int64)), cb.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h)))
        return Prepared(h)

    @staticmethod
    def prepare_for(ctx, M, right, nranks):
        h = C.c_void_p()
        check(lib().blz_prepare_for(ctx.h, C.byref(M.c), C.c_int(int(right)), C.c_int(nranks), C.byref(h)))
        return Prepared(h)

    @staticmethod
    def load(path, key):
        h = C.c_void_p()
        check(lib().blz_prepared_load(path.encode(), C.c_uint64(key), C.byref(h)))
        return Prepared(h)

    def save(self, path, key):
        check(lib().blz_prepared_save(self.h, path.encode(), C.c_uint64(key)))

    def slab(self, rank, t):
        A = Csr()
        check(lib().blz_prepared_slab(self.h, C.c_int(rank), C.c_int(t), C.byref(A)))
        rp = np.ctypeslib.as_array(A.row_ptr, (A.rows + 1,)).copy()
        ci = np.ctypeslib.as_array(A.col_idx, (max(A.nnz, 1),))[:A.nnz].copy()
        va = np.ctypeslib.as_array(A.val, (max(A.nnz, 1),))[:A.nnz].copy() if A.val else np.ones(A.nnz, np.uint32)
        out = dict(rows=int(A.rows), cols=int(A.cols), nnz=int(A.nnz), row_ptr=rp, col_idx=ci, val=va)
        lib().blz_csr_free(C.byref(A))
        return out

    def layout(self):
        """(right, nranks, chunks, bounds of side 0, bounds of side 1, strides)"""
        r, nr, ch = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().blz_prepared_describe(self.h, C.byref(r), C.byref(nr), C.byref(ch)))
        b0 = (C.c_int64 * (nr.value + 1))()
        b1 = (C.c_int64 * (nr.value + 1))()
        st = (C.c_int64 * 2)()
        check(lib().blz_prepared_layout(self.h, b0, b1, st))
        return bool(r.value), nr.value, ch.value, list(b0), list(b1), list(st)

    def slab_short(self, rank, t):
        """blz_prepared_slab_short(): product t in its short-side form for rank `rank`."""
        A = Csr()
        check(lib().blz_prepared_slab_short(self.h, C.c_int(rank), C.c_int(t), C.byref(A)))
        rp = np.ctypeslib.as_array(A.row_ptr, (A.rows + 1,)).copy()
        ci = np.ctypeslib.as_array(A.col_idx, (max(A.nnz, 1),))[:A.nnz].copy()
        va = np.ctypeslib.as_array(A.val, (max(A.nnz, 1),))[:A.nnz].copy() if A.val else np.ones(A.nnz, np.uint32)
        out = dict(rows=int(A.rows), cols=int(A.cols), nnz=int(A.nnz), row_ptr=rp, col_idx=ci, val=va)
        lib().blz_csr_free(C.byref(A))
        return out

    def close(self):
        if self.h:
            lib().blz_prepared_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def prepare_key(ctx, content_hash, M, right, nranks):
    return int(lib().blz_prepare_key(ctx.h, C.c_uint64(content_hash), C.c_int64(M.nrows), C.c_int64(M.ncols), C.c_int64(M.nnz),
                                     C.c_int(int(right)), C.c_int(nranks)))


def file_hash(path):
    return int(lib().blz_file_hash(path.encode()))


def reorder_hot(M, hot_rows, hot_cols, min_share=0.10):
    """blz_reorder_hot(): (row_perm, col_perm, (rows taken, columns taken), (their shares of the entries))."""
    rp = np.empty(M.nrows, dtype=np.int32)
    cp = np.empty(M.ncols, dtype=np.int32)
    hot = (C.c_int64 * 2)(hot_rows, hot_cols)
    share = (C.c_double * 2)(0.0, 0.0)
    check(lib().blz_reorder_hot(C.byref(M.c), rp.ctypes.data_as(C.POINTER(C.c_int32)), cp.ctypes.data_as(C.POINTER(C.c_int32)),
                                hot, C.c_double(min_share), share))
    return rp, cp, (int(hot[0]), int(hot[1])), (float(share[0]), float(share[1]))


def reorder_auto(M, hot_rows=0, hot_cols=0, min_share=0.25, rows_per_line=2):
    """blz_reorder_auto(): (row_perm, col_perm, hot taken, shares, (lines per entry M*x, M^T*x), order kind)."""
    rp = np.empty(M.nrows, dtype=np.int32)
    cp = np.empty(M.ncols, dtype=np.int32)
    hot = (C.c_int64 * 2)(hot_rows, hot_cols)
    share = (C.c_double * 2)(0.0, 0.0)
    loc = (C.c_double * 2)(1.0, 1.0)
    kind = C.c_int(0)
    check(lib().blz_reorder_auto(C.byref(M.c), rp.ctypes.data_as(C.POINTER(C.c_int32)), cp.ctypes.data_as(C.POINTER(C.c_int32)),
                                 hot, C.c_double(min_share), share, C.c_int(rows_per_line), loc, C.byref(kind)))
    return rp, cp, (int(hot[0]), int(hot[1])), (float(share[0]), float(share[1])), (float(loc[0]), float(loc[1])), int(kind.value)


def reorder(M):
    """blz_reorder(): (row_perm, col_perm), new index of every row / column of M."""
    rp = np.zeros(M.nrows, dtype=np.int32)
    cp = np.zeros(M.ncols, dtype=np.int32)
    check(lib().blz_reorder(C.byref(M.c), rp.ctypes.data_as(C.POINTER(C.c_int32)), cp.ctypes.data_as(C.POINTER(C.c_int32))))
    return rp, cp


def rng_draws(count):
    s = (C.c_uint64 * 4)()
    lib().blz_rng_seed(s)
    return [int(lib().blz_rng_next(s)) for _ in range(count)]


def rng_fill(words, prime):
    v = np.zeros(words, dtype=np.uint64)
    check(lib().blz_rng_fill(ptr(v), C.c_int64(words), C.c_uint64(prime)))
    return v


def save_block(path, nrows, n, v):
    check(lib().blz_save_block(path.encode(), C.c_int64(nrows), C.c_int(n), ptr(u64(v))))


def check_kernel(matrix_path, kernel_path, prime, right=False, signed=False, where=False, wide=False):
    """blz_check_kernel(): 0 OK, 1 all-zero kernel, 2 product not zero; raises on file/format errors.
    signed=True: the matrix in signed value mode (blz_check_kernel_signed).  where=True: (rc, row, column), the place
    of the first non-zero word when rc == 2."""
    row, col = C.c_int64(0), C.c_int(0)
    fn = lib().blz_check_kernel_wide if wide else lib().blz_check_kernel_signed if signed else lib().blz_check_kernel
    rc = fn(matrix_path.encode(), kernel_path.encode(), C.c_uint64(prime), C.c_int(int(right)), C.byref(row), C.byref(col))
    if rc < 0:
        check(rc)
    if where:
        return rc, (int(row.value) if rc == 2 else None), (int(col.value) if rc == 2 else None)
    return rc


def check_independent(kernel_path, prime):
    """blz_check_independent(): (rank, columns) of a kernel block file mod prime (host only)."""
    rank, cols = C.c_int(0), C.c_int(0)
    check(lib().blz_check_independent(kernel_path.encode(), C.c_uint64(prime), C.byref(rank), C.byref(cols)))
    return int(rank.value), int(cols.value)


def rhs_load(path, prime, length):
    """blz_rhs_load(): the `length` words of a right-hand side file, signed entries reduced as true residues."""
    b = np.zeros(max(length, 1), dtype=np.uint64)
    check(lib().blz_rhs_load(path.encode(), C.c_uint64(prime), C.c_int64(length), ptr(b)))
    return b[:length]


def check_solution(matrix_path, rhs_path, x_path, prime, right=False, signed=False, wide=False):
    """blz_check_solution(): (0, None) when M x == b (right) / x M == b, else (2, first differing row); raises on
    file / format errors.  signed=True: the matrix in signed value mode."""
    row = C.c_int64(-1)
    fn = lib().blz_check_solution_wide if wide else lib().blz_check_solution_signed if signed else lib().blz_check_solution
    rc = fn(matrix_path.encode(), rhs_path.encode(), x_path.encode(), C.c_uint64(prime), C.c_int(int(right)), C.byref(row))
    if rc < 0:
        check(rc)
    return rc, (int(row.value) if rc == 2 else None)


MAX_RHS = 16


def rhs_load_block(path, prime, length, kmax=MAX_RHS):
    """blz_rhs_load_block(): the length x k words of a file of k right-hand sides, row-major (b[r, i] = entry r of
    right-hand side i), as an array of shape (length, k)."""
    b = np.zeros(max(length, 1) * kmax, dtype=np.uint64)
    k = C.c_int(0)
    check(lib().blz_rhs_load_block(path.encode(), C.c_uint64(prime), C.c_int64(length), C.c_int(kmax), C.byref(k), ptr(b)))
    return b[:length * k.value].reshape(length, k.value)


def check_solution_block(matrix_path, rhs_path, x_path, prime, right=False, signed=False, wide=False):
    """blz_check_solution_block(): one (status, row) per right-hand side -- (0, None) equal, (2, first differing row),
    (3, None) the x column is all zero; raises on file / format errors.  signed=True: the matrix in signed value mode."""
    status = (C.c_int * MAX_RHS)()
    rows = (C.c_int64 * MAX_RHS)()
    fn = (lib().blz_check_solution_block_wide if wide else
          lib().blz_check_solution_block_signed if signed else lib().blz_check_solution_block)
    k = fn(matrix_path.encode(), rhs_path.encode(), x_path.encode(), C.c_uint64(prime), C.c_int(int(right)), status, rows)
    if k < 0:
        check(k)
    return [(int(status[i]), int(rows[i]) if status[i] == 2 else None) for i in range(k)]


def gathered_position(bounds, stride, chunks, row):
    """blz_gathered_position(): (owner, local row, position in the gathered operand) of row `row` (solver's numbering)."""
    bd = np.ascontiguousarray(bounds, dtype=np.int64)
    owner, local = C.c_int(-1), C.c_int64(-1)
    lib().blz_gathered_position.restype = C.c_int64
    pos = int(lib().blz_gathered_position(bd.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(len(bd) - 1), C.c_int64(stride),
                                          C.c_int(chunks), C.c_int64(row), C.byref(owner), C.byref(local)))
    if pos < 0:
        check(pos)
    return int(owner.value), int(local.value), pos


def rhs_cut(b, prime, first, count, kp, perm=None):
    """blz_rhs_cut(): rows [first, first + count) (solver's numbering) of the len x k block b as a count x kp array."""
    b = np.ascontiguousarray(b, dtype=np.uint64)
    out = np.full(max(count, 1) * kp, 0xDEADBEEF, dtype=np.uint64)
    pm = np.ascontiguousarray(perm, dtype=np.int32) if perm is not None else None
    check(lib().blz_rhs_cut(ptr(b.reshape(-1)), C.c_int64(b.shape[0]), C.c_int(b.shape[1]), C.c_int(kp), C.c_uint64(prime),
                            pm.ctypes.data_as(C.POINTER(C.c_int32)) if pm is not None else None, C.c_int64(first),
                            C.c_int64(count), ptr(out)))
    return out[:count * kp].reshape(count, kp)


def checkpoint_save(path, prime, n, right, nrows, iterations, v, p):
    check(lib().blz_checkpoint_save(path.encode(), C.c_uint64(prime), C.c_int(n), C.c_int(int(right)),
                                    C.c_int64(nrows), C.c_int64(iterations), ptr(u64(v)), ptr(u64(p))))


def checkpoint_load(path, prime, n, right, nrows):
    v = np.zeros(nrows * n, dtype=np.uint64)
    p = np.zeros(nrows * n, dtype=np.uint64)
    its = C.c_int64(0)
    check(lib().blz_checkpoint_load(path.encode(), C.c_uint64(prime), C.c_int(n), C.c_int(int(right)),
                                    C.c_int64(nrows), C.byref(its), ptr(v), ptr(p)))
    return int(its.value), v, p


class LoopGroup:
    """blz_loop_group: the loopback communicator of several contexts on one device (one thread per context)."""

    def __init__(self, nranks):
        self.h = C.c_void_p()
        check(lib().blz_loop_group_create(C.c_int(nranks), C.byref(self.h)))
        self.nranks = nranks

    def close(self):
        if self.h:
            lib().blz_loop_group_destroy(self.h)
            self.h = None


class Context:
    """One GPU's solver state: the globals `n` and `prime` of the reference plus its four blocks."""

    def __init__(self, prime, n, device=0):
        self.h = C.c_void_p()
        self.prime, self.n, self.device = int(prime), int(n), int(device)
        check(lib().blz_create(C.byref(self.h), C.c_int(device), C.c_uint64(prime), C.c_int(n)))

    def close(self):
        if self.h:
            lib().blz_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def word_bytes(self):
        return int(lib().blz_word_bytes(self.h))

    def set_values_signed(self, on=True):
        """blz_set_values_signed(): signed value mode -- the x of every matrix set afterwards is an int32 bit pattern
        (Matrix.load_signed) and an entry a means a mod p.  Before the matrix is set."""
        check(lib().blz_set_values_signed(self.h, C.c_int(int(bool(on)))))

    def values_signed(self):
        return bool(lib().blz_values_signed(self.h))

    def slab_signed(self, transpose, piece=0):
        """blz_slab_signed(): True when that slab's products run the signed instantiations of the SpMV kernels."""
        rc = int(lib().blz_slab_signed(self.h, C.c_int(int(transpose)), C.c_int(piece)))
        if rc < 0:
            check(rc)
        return bool(rc)

    def set_values_wide(self, x_hi, nnz=None):
        """blz_set_values_wide(): the high limbs of the next matrix's entries (None clears the mode)."""
        if x_hi is None:
            check(lib().blz_set_values_wide(self.h, None, C.c_int64(0)))
            return
        x_hi = np.ascontiguousarray(x_hi, dtype=np.uint32)
        self._x_hi = x_hi       # borrowed by the library until the matrix is set
        check(lib().blz_set_values_wide(self.h, x_hi.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        C.c_int64(x_hi.size if nnz is None else nnz)))

    def values_wide(self):
        return bool(lib().blz_values_wide(self.h))

    def slab_wide(self, transpose, piece=0):
        """blz_slab_wide(): True when that slab's products run the wide instantiations of the SpMV kernels."""
        rc = int(lib().blz_slab_wide(self.h, C.c_int(int(transpose)), C.c_int(piece)))
        if rc < 0:
            check(rc)
        return bool(rc)

    def _hand_over_wide(self, M):
        if getattr(M, "x_hi", None) is not None:
            self.set_values_wide(M.x_hi)

    def set_matrix(self, M, right=False, rank=0, nranks=1):
        self._hand_over_wide(M)
        check(lib().blz_set_matrix(self.h, C.byref(M.c), C.c_int(int(right)), C.c_int(rank), C.c_int(nranks)))
        self.right = bool(right)

    # ---- device matrix: the triplets are torch tensors on the context's device; torch is imported inside these methods only

    @staticmethod
    def _matrix_dims(i, j, nrows, ncols, who):
        """(nrows, ncols) of a matrix of device triplets: what is not given is 1 + the largest index (a device reduction)"""
        if nrows is None or ncols is None:
            if tuple(i.shape)[0] == 0:
                raise ValueError(f"{who}: an empty matrix needs nrows and ncols")
            nrows = int(i.max()) + 1 if nrows is None else nrows
            ncols = int(j.max()) + 1 if ncols is None else ncols
        return nrows, ncols

    def set_matrix_device(self, i, j, x=None, nrows=None, ncols=None, right=False, stream=None, reorder=False):
        """blz_set_matrix_device(): M from triplets on the GPU (device_triplets() says what i, j, x may be); both CSRs are
        built there and the caller's numbering is kept.  nrows / ncols default to 1 + the largest index (a device
        reduction; an empty matrix needs them given).  Ordered on `stream` (default: torch's current stream); synchronises.
        reorder=True: blz_set_matrix_device_ordered() with order 1 -- rows and columns are renumbered on the GPU first
        (blz_reorder's order); nothing of the numbering shows."""
        pi, pj, ib, px, vb, nnz = device_triplets(i, j, x, self.device)
        nrows, ncols = self._matrix_dims(i, j, nrows, ncols, "set_matrix_device")
        args = (self.h, C.c_int64(nrows), C.c_int64(ncols), C.c_int64(nnz), C.c_void_p(pi), C.c_void_p(pj), C.c_int(ib),
                C.c_void_p(px), C.c_int(vb), C.c_int(int(bool(right))))
        if reorder:
            check(lib().blz_set_matrix_device_ordered(*args, C.c_int(int(reorder)), C.c_void_p(self._stream(stream))))
        else:
            check(lib().blz_set_matrix_device(*args, C.c_void_p(self._stream(stream))))
        self.right = bool(right)

    def set_matrix_sparse(self, t, right=False, stream=None, reorder=False):
        """set_matrix_device() of a 2-D torch sparse COO tensor: rows 0 and 1 of its _indices() and its _values(), dimensions
        from t.shape.  The tensor need not be coalesced: duplicates add up."""
        if len(tuple(t.shape)) != 2:
            raise ValueError(f"set_matrix_sparse: {len(tuple(t.shape))} dimensions, a matrix has 2")
        idx, val = t._indices(), t._values()
        if not idx.is_contiguous():
            idx = idx.contiguous()
        self.set_matrix_device(idx[0], idx[1], val.contiguous(), nrows=int(t.shape[0]), ncols=int(t.shape[1]), right=right,
                               stream=stream, reorder=reorder)

    def set_matrix_upload(self, M, right=False, reorder=False):
        """blz_set_matrix_upload(): the host triplets of M through the device build (numbering kept, as set_matrix_device;
        reorder=True: blz_set_matrix_upload_ordered() with order 1)."""
        if getattr(M, "x_hi", None) is not None:
            raise ValueError("set_matrix_upload: wide entries go through set_matrix_device as 8-byte values")
        if reorder:
            check(lib().blz_set_matrix_upload_ordered(self.h, C.byref(M.c), C.c_int(int(bool(right))), C.c_int(int(reorder))))
        else:
            check(lib().blz_set_matrix_upload(self.h, C.byref(M.c), C.c_int(int(bool(right)))))
        self.right = bool(right)

    def matrix_device_built(self):
        return bool(lib().blz_matrix_device_built(self.h))

    def matrix_device_order(self):
        """blz_matrix_device_order(): 1 when the resident matrix was renumbered and built on the device, else 0"""
        return int(lib().blz_matrix_device_order(self.h))

    def numbering(self, block):
        """blz_numbering() (a test hook): (resident, perm) -- perm[r] = the solver's index of original row r of the block's
        side, an int32 array of rows(block) words; resident False: the identity"""
        perm = np.zeros(max(self.rows(block), 0), dtype=np.int32)
        rc = lib().blz_numbering(self.h, C.c_int(block), perm.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc < 0:
            check(rc)
        return bool(rc), perm

    def set_matrix_prepared(self, P, rank=0):
        check(lib().blz_set_matrix_prepared(self.h, P.h, C.c_int(rank)))
        r = C.c_int(0)
        check(lib().blz_prepared_describe(P.h, C.byref(r), None, None))
        self.right = bool(r.value)

    def set_matrix_rhs(self, M, b, right=False):
        """blz_set_matrix_rhs(): M x = b (right; b has M.nrows words) or x M = b (b has M.ncols words) as the bordered
        operator; rows(V) then counts the border row."""
        b = u64(b)
        assert b.size == (M.nrows if right else M.ncols), (b.size, M.nrows, M.ncols, right)
        self._hand_over_wide(M)
        check(lib().blz_set_matrix_rhs(self.h, C.byref(M.c), C.c_int(int(right)), ptr(b)))
        self.right = bool(right)

    def set_rhs(self, b):
        """blz_set_rhs(): the border for a matrix already set with the extra empty last row / column."""
        b = u64(b)
        assert b.size == self.rows(TMP), (b.size, self.rows(TMP))
        check(lib().blz_set_rhs(self.h, ptr(b)))

    @property
    def has_rhs(self):
        return bool(lib().blz_has_rhs(self.h))

    def solution(self):
        """blz_solution(): (status, x) -- x is None unless status == 0 (1: no solution found, 2: verification failed)."""
        x = np.zeros(max(self.rows(V) - 1, 1), dtype=np.uint64)
        status = C.c_int(-1)
        check(lib().blz_solution(self.h, ptr(x), C.byref(status)))
        return int(status.value), (x[:self.rows(V) - 1] if status.value == 0 else None)

    @staticmethod
    def _rhs_block(b, rows):
        """b as the block and ranks setters hand it over: contiguous uint64, rows x k"""
        b = np.ascontiguousarray(b, dtype=np.uint64)
        assert b.ndim == 2 and b.shape[0] == rows, (b.shape, rows)
        return b

    def set_matrix_rhs_block(self, M, b, right=False):
        """blz_set_matrix_rhs_block(): M X = B (right; B is M.nrows x k) or X M = B (B is M.ncols x k), k right-hand sides
        in one bordered operator; rows(V) then counts the k border rows."""
        b = self._rhs_block(b, M.nrows if right else M.ncols)
        self._hand_over_wide(M)
        check(lib().blz_set_matrix_rhs_block(self.h, C.byref(M.c), C.c_int(int(right)), C.c_int(b.shape[1]), ptr(b.reshape(-1))))
        self.right = bool(right)

    def set_rhs_block(self, b):
        """blz_set_rhs_block(): the k borders for a matrix already set with the k extra empty last rows / columns."""
        b = self._rhs_block(b, self.rows(TMP))
        check(lib().blz_set_rhs_block(self.h, C.c_int(b.shape[1]), ptr(b.reshape(-1))))

    def set_matrix_rhs_ranks(self, M, b, right=False, rank=0, nranks=1):
        """blz_set_matrix_rhs_ranks(): the bordered operator of set_matrix_rhs_block row-partitioned over nranks ranks (attach
        the communicator first); b is the WHOLE block (M.nrows x k resp. M.ncols x k) on every rank.  Collective."""
        b = self._rhs_block(b, M.nrows if right else M.ncols)
        check(lib().blz_set_matrix_rhs_ranks(self.h, C.byref(M.c), C.c_int(int(right)), C.c_int(b.shape[1]), ptr(b.reshape(-1)),
                                             C.c_int(rank), C.c_int(nranks)))
        self.right = bool(right)

    def set_rhs_ranks(self, b):
        """blz_set_rhs_ranks(): the k borders for a matrix this rank has set with the k extra empty last rows / columns; b is
        the whole rows(TMP) x k block on every rank.  Collective."""
        b = self._rhs_block(b, self.rows(TMP))
        check(lib().blz_set_rhs_ranks(self.h, C.c_int(b.shape[1]), ptr(b.reshape(-1))))

    @property
    def rhs_count(self):
        return int(lib().blz_rhs_count(self.h))

    def solution_block(self):
        """blz_solution_block(): (statuses, x) -- statuses[i] is 0 (solved and verified), 1 (not solved, column i of x
        zero) or 2 (verification failed: x is None); x has shape (rows(V) - k, k)."""
        k = self.rhs_count
        length = self.rows(V) - k
        x = np.zeros(max(length * k, 1), dtype=np.uint64)
        status = (C.c_int * MAX_RHS)(*([-1] * MAX_RHS))
        check(lib().blz_solution_block(self.h, ptr(x), status))
        st = [int(status[i]) for i in range(k)]
        return st, (None if 2 in st else x[:length * k].reshape(length, k))

    # ---- device right-hand sides: b and x are torch tensors on the context's device; torch is imported inside these methods only

    def _set_rhs_device(self, read, fn, b, stream):
        rows = self.rows(TMP)       # (0 without a matrix: the library says so)
        p, _, k, ld = read(b, self.n, rows if rows > 0 else None, self.device)
        check(fn(self.h, C.c_int(k), C.c_void_p(p), C.c_int64(ld), C.c_void_p(self._stream(stream))))

    def set_rhs_device(self, b, stream=None):
        """blz_set_rhs_device(): set_rhs_block() (set_rhs() for one column) from a tensor on the GPU -- device_rhs() says what
        b may be: (rows(TMP),) or (rows(TMP), k), uint64 / int64, any row stride.  The matrix is already set with its k empty
        last rows / columns.  Ordered on `stream` (default: torch's current stream); validates and synchronises."""
        self._set_rhs_device(device_rhs, lib().blz_set_rhs_device, b, stream)

    def set_rhs_device32(self, b, stream=None):
        """blz_set_rhs_device32(): set_rhs_device() from a tensor of 32-bit words (uint32 / int32; p < 2**32)."""
        self._set_rhs_device(device_rhs32, lib().blz_set_rhs_device32, b, stream)

    def _solution_device(self, read, dtype, fn, out, stream):
        k = self.rhs_count
        if k < 1:
            raise ValueError("solution_device: the context has no right-hand side")
        length = self.rows(V) - k
        if out is None:
            import torch
            # (zeroed through the signed dtype of the same width: fills of the unsigned ones are not everywhere in torch)
            out = torch.zeros((length, k), dtype=getattr(torch, dtype[1:]), device=f"cuda:{self.device}").view(getattr(torch, dtype))
        p, _, kk, ld = read(out, self.n, length, self.device)
        if kk != k:
            raise ValueError(f"solution_device: out has {kk} columns, the context {k} right-hand sides")
        status = (C.c_int * MAX_RHS)(*([-1] * MAX_RHS))
        check(fn(self.h, C.c_void_p(p), C.c_int64(ld), status, C.c_void_p(self._stream(stream))))
        return [int(status[i]) for i in range(k)], out

    def solution_device(self, out=None, stream=None):
        """blz_solution_device(): (statuses, x) as solution_block() gives them, x a (rows(V) - k, k) tensor on the GPU: `out`
        (uint64 / int64, any row stride; words past k of a row are not written) or a new torch.uint64 one.  Columns of
        unsolved systems are zero; when the verification fails every status is 2 and x is as it was (zero when new)."""
        return self._solution_device(device_rhs, "uint64", lib().blz_solution_device, out, stream)

    def solution_device32(self, out=None, stream=None):
        """blz_solution_device32(): solution_device() into a tensor of 32-bit words (a new torch.uint32 one when not given)."""
        return self._solution_device(device_rhs32, "uint32", lib().blz_solution_device32, out, stream)

    def set_matrix_rhs_device(self, i, j, x, b, nrows=None, ncols=None, right=False, stream=None, reorder=False):
        """set_matrix_device() with the dimension raised by k, then set_rhs_device(): M x = b (right; b has nrows rows) or
        x M = b (b has ncols rows) from triplets and right-hand sides that all live on the GPU."""
        nrows, ncols = self._matrix_dims(i, j, nrows, ncols, "set_matrix_rhs_device")
        k = device_rhs(b, self.n, nrows if right else ncols, self.device)[2]
        self.set_matrix_device(i, j, x, nrows + (0 if right else k), ncols + (k if right else 0), right, stream, reorder)
        self.set_rhs_device(b, stream)

    def rows(self, block):
        return int(lib().blz_rows(self.h, C.c_int(block)))

    def local_rows(self, block):
        first = C.c_int64(0)
        cnt = int(lib().blz_local_rows(self.h, C.c_int(block), C.byref(first)))
        return int(first.value), cnt

    def local_nnz(self, transpose):
        return int(lib().blz_local_nnz(self.h, C.c_int(int(transpose))))

    def matrix_stream_bytes(self, transpose):
        return int(lib().blz_matrix_stream_bytes(self.h, C.c_int(int(transpose))))

    def locality(self):
        """((lines per gathered entry of M*x, of M^T*x), order kind) as found by the renumbering (blz_locality)."""
        loc = (C.c_double * 2)(1.0, 1.0)
        kind = C.c_int(0)
        check(lib().blz_locality(self.h, loc, C.byref(kind)))
        return (float(loc[0]), float(loc[1])), int(kind.value)

    def comm_init_loopback(self, group, rank):
        check(lib().blz_comm_init_loopback(self.h, group.h, C.c_int(rank)))

    def comm_info(self):
        """(ranks, rank) as the RCCL communicator reports them; (-1, -1) without one"""
        a, b = C.c_int(-1), C.c_int(-1)
        check(lib().blz_comm_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def exchange_pieces_for(self, mrows, mcols, nnz, nranks):
        return int(lib().blz_exchange_pieces_for(self.h, C.c_int64(mrows), C.c_int64(mcols), C.c_int64(nnz), C.c_int(nranks)))

    def exchange_pieces(self, transpose):
        return int(lib().blz_exchange_pieces(self.h, C.c_int(1 if transpose else 0)))

    def short_side(self, transpose):
        return bool(lib().blz_short_side(self.h, C.c_int(int(transpose))) == 1)

    def get_partial(self, transpose):
        rows = self.rows(TMP) if bool(transpose) == (not self.right) else self.rows(V)
        out = np.zeros(rows * self.n, dtype=np.uint64)
        check(lib().blz_get_partial(self.h, C.c_int(int(transpose)), ptr(out)))
        return out

    def panel_rows(self, transpose):
        """(block rows of the operand kept in LDS, share of the entries they serve) for M*x (False) / M^T*x (True)."""
        share = C.c_double(0.0)
        rows = int(lib().blz_panel_rows(self.h, C.c_int(int(transpose)), C.byref(share)))
        return rows, float(share.value)

    def plan(self, transpose, piece=0):
        """blz_slab_plan(): what the launches of product M*x (False) / M^T*x (True), column piece `piece`, will be, as
        a dict; "plain" and "dot" are dicts of their own (form: "spmv" / "staged" / "panel", the four grids, ...)."""
        out = Plan()
        check(lib().blz_slab_plan(self.h, C.c_int(int(transpose)), C.c_int(piece), C.byref(out)))
        res = {}
        for name, _ in Plan._fields_:
            val = getattr(out, name)
            if isinstance(val, PlanLaunch):
                val = {k: getattr(val, k) for k, _ in PlanLaunch._fields_}
                val["form"] = FORMS[val["form"]]
            res[name] = val
        return res

    def devalg_plan(self, op, rows, nterms=1, aligned=True):
        """blz_devalg_plan(): which kernels the device block algebra call `op` (DEVOP_DOT, DEVOP_DOT_PAIR, DEVOP_COMBINE,
        DEVOP_COMBINE_PAIR) will run for `rows` rows and `nterms` terms, on blocks that all have a 16-byte aligned base and an
        even ld (aligned) or not, as a dict: form (0 vector ALU, 1 matrix cores), min_rows, tile_rows, wavefronts, fold_tiles,
        lds_bytes.  Nothing is launched; no matrix is needed."""
        out = DevalgPlan()
        check(lib().blz_devalg_plan(self.h, C.c_int(int(op)), C.c_int64(int(rows)), C.c_int(int(nterms)),
                                    C.c_int(1 if aligned else 0), C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in DevalgPlan._fields_}

    def owner_of_row(self, block, row):
        return int(lib().blz_owner_of_row(self.h, C.c_int(block), C.c_int64(row)))

    def init_v(self):
        check(lib().blz_init_v(self.h))

    def set_block(self, block, host):
        host = u64(host)
        assert host.size == self.rows(block) * self.n, (host.size, self.rows(block), self.n)
        check(lib().blz_set_block(self.h, C.c_int(block), ptr(host)))

    def get_block(self, block):
        out = np.zeros(self.rows(block) * self.n, dtype=np.uint64)
        check(lib().blz_get_block(self.h, C.c_int(block), ptr(out)))
        return out

    # ---- device blocks: torch tensors (uint64 or int64) on the context's device; torch is imported here and only here

    def _stream(self, stream):
        if stream is None:
            import torch
            return int(torch.cuda.current_stream(self.device).cuda_stream)
        return int(getattr(stream, "cuda_stream", stream))

    def _new_block(self, rows, like=None):
        """a block the wrapper allocates: torch.uint64 whatever `like` is (_new_block32 takes its dtype from it)"""
        import torch
        return torch.empty((rows, self.n), dtype=torch.uint64, device=f"cuda:{self.device}")

    # ---- device blocks on ranks: with device_ranks() the blocks of every method below are the rank's own rows, in slab order

    def device_ranks(self, on=True):
        """blz_set_device_ranks(): device blocks are rank-local from here on (every rank of a job alike); returns self."""
        check(lib().blz_set_device_ranks(self.h, C.c_int(1 if on else 0)))
        return self

    @property
    def device_ranks_on(self):
        return bool(lib().blz_device_ranks(self.h))

    def _block_rows(self, block):
        """rows of a device block of `block`: the rank's own with the mode on, all of them otherwise"""
        return self.local_rows(block)[1] if self.device_ranks_on else self.rows(block)

    def local_row_ids(self, block):
        """blz_local_row_ids(): the original row number of every local row of `block`, int64 numpy (a host call)."""
        ids = np.zeros(max(self.local_rows(block)[1], 0), dtype=np.int64)
        check(lib().blz_local_row_ids(self.h, C.c_int(block), ids.ctypes.data_as(C.POINTER(C.c_int64))))
        return ids

    def take_local(self, block, whole, out=None, stream=None):
        """blz_take_local_device(): out <- this rank's rows of `whole`, a (rows(block), n) tensor in the original numbering;
        out is (local rows, n), a new torch.uint64 tensor when not given.  Not collective."""
        rows = self.rows(block) if 0 <= block <= 3 else None
        local = self.local_rows(block)[1] if 0 <= block <= 3 else None
        pw, _, ldw, _ = device_block(whole, self.n, rows, self.device)
        if out is None:
            out = self._new_block(local if local is not None else 1)
        pl, _, ldl, _ = device_block(out, self.n, local, self.device)
        check(lib().blz_take_local_device(self.h, C.c_int(block), C.c_void_p(pw), C.c_int64(ldw), C.c_void_p(pl), C.c_int64(ldl),
                                          C.c_void_p(self._stream(stream))))
        return out

    def put_local(self, block, local, whole, stream=None):
        """blz_put_local_device(): this rank's rows of `whole` <- local; no other row of `whole` is touched.  Returns whole."""
        rows = self.rows(block) if 0 <= block <= 3 else None
        count = self.local_rows(block)[1] if 0 <= block <= 3 else None
        pl, _, ldl, _ = device_block(local, self.n, count, self.device)
        pw, _, ldw, _ = device_block(whole, self.n, rows, self.device)
        check(lib().blz_put_local_device(self.h, C.c_int(block), C.c_void_p(pl), C.c_int64(ldl), C.c_void_p(pw), C.c_int64(ldw),
                                         C.c_void_p(self._stream(stream))))
        return whole

    # ---- what a method and its ...32 namesake share: `read` is device_block or device_block32, `new` the allocator of a block
    # the wrapper makes (_new_block or _new_block32: rows, and the block whose dtype a 32-bit one takes), `fn` the C function

    def _dev_set(self, read, fn, block, t, validate, stream):
        rows = self._block_rows(block) if 0 <= block <= 3 else None
        p, _, ld, _ = read(t, self.n, rows, self.device)
        bad = C.c_int64(-1)
        check(fn(self.h, C.c_int(block), C.c_void_p(p), C.c_int64(ld), C.c_void_p(self._stream(stream)),
                 C.byref(bad) if validate else None))
        return int(bad.value) if validate else None

    def _dev_get(self, read, new, fn, block, out, stream):
        rows = self._block_rows(block) if 0 <= block <= 3 else None
        if out is None:
            out = new(rows if rows is not None else 1)
        p, _, ld, _ = read(out, self.n, rows, self.device)
        check(fn(self.h, C.c_int(block), C.c_void_p(p), C.c_int64(ld), C.c_void_p(self._stream(stream))))
        return out

    def _dev_apply(self, read, new, fn, transpose, x, out, stream):
        xr, yr = self.apply_rows(transpose)
        px, _, ldx, _ = read(x, self.n, xr, self.device)
        if out is None:
            out = new(yr, x)
        py, _, ldy, _ = read(out, self.n, yr, self.device)
        check(fn(self.h, C.c_int(int(bool(transpose))), C.c_void_p(px), C.c_int64(ldx), C.c_void_p(py), C.c_int64(ldy),
                 C.c_void_p(self._stream(stream))))
        return out

    def _dev_apply_pair(self, read, new, fn, transpose_first, x, out, mid, stream):
        xr, yr = self.apply_rows(transpose_first)
        px, _, ldx, _ = read(x, self.n, xr, self.device)
        if out is None:
            out = new(xr, x)
        pz, _, ldz, _ = read(out, self.n, xr, self.device)
        if mid is True:
            mid = new(yr, x)
        py, ldy = None, 0
        if mid is not None:
            py, _, ldy, _ = read(mid, self.n, yr, self.device)
        check(fn(self.h, C.c_int(int(bool(transpose_first))), C.c_void_p(px), C.c_int64(ldx), C.c_void_p(py), C.c_int64(ldy),
                 C.c_void_p(pz), C.c_int64(ldz), C.c_void_p(self._stream(stream))))
        return out if mid is None else (out, mid)

    def _dev_dot(self, read, fn, xs, y, out, stream):
        """x^T y for each x of xs, one or two: out is (n, n) for one, (2, n, n) for two"""
        rows, args = None, []
        for x in xs + (y,):
            px, rows, ldx, _ = read(x, self.n, rows, self.device)
            args += [C.c_void_p(px), C.c_int64(ldx)]
        if out is None:
            out = self._empty((self.n, self.n) if len(xs) == 1 else (2, self.n, self.n))
        pc = device_square(out, self.n, self.device) if len(xs) == 1 else device_pair(out, self.n, self.device)
        check(fn(self.h, C.c_int64(rows), *args, C.c_void_p(pc), C.c_void_p(self._stream(stream))))
        return out

    def _dev_combine(self, read, new, fn, terms, out, stream):
        terms = list(terms)
        if not 1 <= len(terms) <= MAX_TERMS:
            raise ValueError(f"combine: {len(terms)} terms, not 1..{MAX_TERMS}")
        terms = [(pair[0], self._coefficient(pair[1], stream)) for pair in terms]
        rows, args = device_terms(terms, self.n, self.device, read)
        if out is None:
            out = new(rows, terms[0][0])
        pz, _, ldz, _ = read(out, self.n, rows, self.device)
        k = len(args)
        xs = (C.c_void_p * k)(*[a[0] for a in args])
        lds = (C.c_int64 * k)(*[a[1] for a in args])
        cs = (C.c_void_p * k)(*[a[2] for a in args])
        check(fn(self.h, C.c_int64(rows), C.c_int(k), xs, lds, cs, C.c_void_p(pz), C.c_int64(ldz),
                 C.c_void_p(self._stream(stream))))
        return out

    def _dev_combine_pair(self, read, new, fn, terms, out, stream):
        terms = [tuple(t) for t in terms]
        if not 1 <= len(terms) <= MAX_TERMS:
            raise ValueError(f"combine_pair: {len(terms)} terms, not 1..{MAX_TERMS}")
        terms = [t if len(t) != 3 else (t[0],) + tuple(None if a is None else self._coefficient(a, stream) for a in t[1:])
                 for t in terms]
        rows, args = device_pair_terms(terms, self.n, self.device, read)
        if out is None:
            out = (new(rows, terms[0][0]), new(rows, terms[0][0]))
        (pz0, ldz0), (pz1, ldz1) = device_pair_out(out, self.n, rows, self.device, read)
        k = len(args)
        xs = (C.c_void_p * k)(*[a[0] for a in args])
        lds = (C.c_int64 * k)(*[a[1] for a in args])
        c0 = (C.c_void_p * k)(*[a[2] for a in args])
        c1 = (C.c_void_p * k)(*[a[3] for a in args])
        check(fn(self.h, C.c_int64(rows), C.c_int(k), xs, lds, c0, c1, C.c_void_p(pz0), C.c_int64(ldz0), C.c_void_p(pz1),
                 C.c_int64(ldz1), C.c_void_p(self._stream(stream))))
        return out[0], out[1]

    def set_block_device(self, block, t, validate=False, stream=None):
        """blz_set_block_device(): block <- the tensor t, (rows(block), n) with strides (ld, 1) or flat, ordered on `stream`
        (default: torch's current stream) without a host synchronisation.  validate=True counts the words that are not
        below p (synchronises) and returns the count, 0; a count that is not 0 raises BlzError(EINVAL) with it.
        (With device_ranks() the tensor is the rank's own rows, here and in get_block_device.)"""
        return self._dev_set(device_block, lib().blz_set_block_device, block, t, validate, stream)

    def get_block_device(self, block, out=None, stream=None):
        """blz_get_block_device(): the block as a tensor on the device (out, or a new (rows, n) torch.uint64 one)."""
        return self._dev_get(device_block, self._new_block, lib().blz_get_block_device, block, out, stream)

    def apply_rows(self, transpose):
        """blz_apply_rows(): (rows of x, rows of y) of y = M x (transpose False) / M^T x."""
        xr, yr = C.c_int64(0), C.c_int64(0)
        check(lib().blz_apply_rows(self.h, C.c_int(int(bool(transpose))), C.byref(xr), C.byref(yr)))
        return int(xr.value), int(yr.value)

    def apply(self, transpose, x, out=None, stream=None):
        """blz_apply_device(): out = M x (transpose False) / M^T x on tensors of the context's device, ordered on `stream`;
        the blocks and the state of a solve are left alone.  Returns out (a new torch.uint64 tensor when not given)."""
        return self._dev_apply(device_block, self._new_block, lib().blz_apply_device, transpose, x, out, stream)

    def apply_release(self):
        """blz_apply_release(): free the two scratch slabs apply() works in (they come back on the next call)."""
        check(lib().blz_apply_release(self.h))

    # ---- device block algebra: X^T Y and sum X_t A_t on tensors of the context's device; no matrix needed, no solve touched

    def _coefficient(self, a, stream):
        """an n x n coefficient as a tensor on the device: a tensor is taken as it is (device_square judges it), a numpy array
        or a nested list of residues is moved there on `stream`"""
        import torch
        if isinstance(a, torch.Tensor):
            return a
        host = np.ascontiguousarray(np.array(a, dtype=np.uint64))
        if host.size != self.n * self.n:
            raise ValueError(f"n x n operand: {host.size} words, not {self.n} x {self.n}")
        s = stream if isinstance(stream, torch.cuda.Stream) else \
            torch.cuda.ExternalStream(self._stream(stream), device=f"cuda:{self.device}")
        with torch.cuda.stream(s):
            return torch.from_numpy(host.reshape(self.n, self.n).view(np.int64)).to(f"cuda:{self.device}")

    def dot(self, x, y, out=None, stream=None):
        """blz_dot_device(): out = x^T y mod p, an (n, n) torch.uint64 tensor on the device (out, or a new one); x and y are
        blocks of the same number of rows (any, 0 included), `x is y` gives the Gram matrix.  Ordered on `stream`."""
        return self._dev_dot(device_block, lib().blz_dot_device, (x,), y, out, stream)

    def combine(self, terms, out=None, stream=None):
        """blz_combine_device(): out = sum of X @ A mod p over the 1..4 pairs (X, A) of `terms`, row by row.  X: blocks of the
        same number of rows; A: (n, n) tensors on the device, or numpy arrays / nested lists of residues, which are moved
        there on `stream`.  out: a new (rows, n) torch.uint64 tensor, the caller's, or one of the X (the in-place form)."""
        return self._dev_combine(device_block, self._new_block, lib().blz_combine_device, terms, out, stream)

    # ---- fused device calls: op2 (op1 x), two inner products against one block, two recombinations of shared inputs

    def apply_pair(self, transpose_first, x, out=None, mid=None, stream=None):
        """blz_apply_pair_device(): z = M^T (M x) (transpose_first False) / M (M^T x) in one call.  Returns z (out, or a new
        torch.uint64 tensor; out=x is the in-place form).  mid=True allocates the intermediate, a tensor for mid receives
        it; either way the return is (z, mid).  mid=None: the intermediate never leaves the library's scratch."""
        return self._dev_apply_pair(device_block, self._new_block, lib().blz_apply_pair_device, transpose_first, x, out, mid,
                                    stream)

    def dot_pair(self, x0, x1, y, out=None, stream=None):
        """blz_dot_pair_device(): out[0] = x0^T y and out[1] = x1^T y mod p in one pass, a contiguous (2, n, n) torch.uint64
        tensor on the device (out, or a new one) whose two views go straight into ortho_coeffs.  Blocks that are the same
        tensor are read once."""
        return self._dev_dot(device_block, lib().blz_dot_pair_device, (x0, x1), y, out, stream)

    def combine_pair(self, terms, out=None, stream=None):
        """blz_combine_pair_device(): (z0, z1) with z0 = sum of X @ A0 and z1 = sum of X @ A1 mod p over the 1..4 triples
        (X, A0, A1) of `terms`, every X read once; A0 or A1 may be None (the term does not enter that output).  Coefficients
        as in combine().  out: (z0, z1), each a new block, the caller's, or one of the X (the in-place form), or None."""
        return self._dev_combine_pair(device_block, self._new_block, lib().blz_combine_pair_device, terms, out, stream)

    # ---- 32-bit device blocks: the methods above on torch.uint32 / torch.int32 tensors, for contexts with word_bytes == 4
    # (p < 2**32).  A block the wrapper allocates takes the dtype of the first block passed in (torch.uint32 where there is
    # none); the n x n results are torch.uint64 and the coefficients are what combine() takes, so ortho_coeffs() and
    # semi_inverse_device() serve both families.

    def _new_block32(self, rows, like=None):
        import torch
        return torch.empty((rows, self.n), dtype=like.dtype if like is not None else torch.uint32, device=f"cuda:{self.device}")

    def set_block_device32(self, block, t, validate=False, stream=None):
        """blz_set_block_device32(): set_block_device() from a tensor of 32-bit words."""
        return self._dev_set(device_block32, lib().blz_set_block_device32, block, t, validate, stream)

    def get_block_device32(self, block, out=None, stream=None):
        """blz_get_block_device32(): the block as a tensor of 32-bit words (out, or a new (rows, n) torch.uint32 one)."""
        return self._dev_get(device_block32, self._new_block32, lib().blz_get_block_device32, block, out, stream)

    def apply32(self, transpose, x, out=None, stream=None):
        """blz_apply_device32(): apply() on tensors of 32-bit words.  Returns out (a new tensor of x's dtype when not given)."""
        return self._dev_apply(device_block32, self._new_block32, lib().blz_apply_device32, transpose, x, out, stream)

    def apply_pair32(self, transpose_first, x, out=None, mid=None, stream=None):
        """blz_apply_pair_device32(): apply_pair() on tensors of 32-bit words; out, mid and the return as there."""
        return self._dev_apply_pair(device_block32, self._new_block32, lib().blz_apply_pair_device32, transpose_first, x, out,
                                    mid, stream)

    def dot32(self, x, y, out=None, stream=None):
        """blz_dot_device32(): dot() of two blocks of 32-bit words; out is (n, n) torch.uint64, as there."""
        return self._dev_dot(device_block32, lib().blz_dot_device32, (x,), y, out, stream)

    def dot_pair32(self, x0, x1, y, out=None, stream=None):
        """blz_dot_pair_device32(): dot_pair() of blocks of 32-bit words; out is (2, n, n) torch.uint64, as there."""
        return self._dev_dot(device_block32, lib().blz_dot_pair_device32, (x0, x1), y, out, stream)

    def combine32(self, terms, out=None, stream=None):
        """blz_combine_device32(): combine() on blocks of 32-bit words.  The coefficients are what combine() takes ((n, n)
        uint64 / int64 tensors, numpy arrays, nested lists); out: a new block of the first X's dtype, the caller's, or one
        of the X (the in-place form)."""
        return self._dev_combine(device_block32, self._new_block32, lib().blz_combine_device32, terms, out, stream)

    def combine_pair32(self, terms, out=None, stream=None):
        """blz_combine_pair_device32(): combine_pair() on blocks of 32-bit words; terms, out and the return as there."""
        return self._dev_combine_pair(device_block32, self._new_block32, lib().blz_combine_pair_device32, terms, out, stream)

    # ---- device small algebra: the n x n chain of a Krylov step and the echelon form of a block, results on the device

    def _empty(self, shape, dtype=None):
        import torch
        return torch.empty(shape, dtype=dtype or torch.uint64, device=f"cuda:{self.device}")

    def semi_inverse_device(self, vtav, stream=None):
        """blz_semi_inverse_device(): (winv (n, n), d (n,), npiv (1,)) as torch.uint64 tensors on the device, the reference's
        semi_inverse() of the (n, n) tensor vtav.  Ordered on `stream`; nothing is read on the host."""
        n = self.n
        pa = device_square(vtav, n, self.device)
        winv, d, npiv = self._empty((n, n)), self._empty((n,)), self._empty((1,))
        check(lib().blz_semi_inverse_device(self.h, C.c_void_p(pa), C.c_void_p(winv.data_ptr()), C.c_void_p(d.data_ptr()),
                                            C.c_void_p(npiv.data_ptr()), C.c_void_p(self._stream(stream))))
        return winv, d, npiv

    def ortho_coeffs(self, vtav, vtaav, out=None, stream=None):
        """blz_ortho_coeffs_device(): (coef, npiv) -- coef (5, n, n) contiguous torch.uint64 (out, or a new one), so that
        coef[COEF_V_AV] ... coef[COEF_P_V] go straight into combine(); npiv (1,) on the device.  One launch."""
        n = self.n
        pa, pb = device_square(vtav, n, self.device), device_square(vtaav, n, self.device)
        if out is None:
            out = self._empty((COEF_PANELS, n, n))
        pc = device_coef(out, n, self.device)
        npiv = self._empty((1,))
        check(lib().blz_ortho_coeffs_device(self.h, C.c_void_p(pa), C.c_void_p(pb), C.c_void_p(pc), C.c_void_p(npiv.data_ptr()),
                                            C.c_void_p(self._stream(stream))))
        return out, npiv

    def rref(self, x, null=True, stream=None):
        """blz_rref_device(): (e, z or None, info) of the block x -- e (n, n) the canonical RREF of its row space, z (n, n)
        the canonical null basis of e (null=True), info (n + 1,) torch.int64 = [rank, pivot columns, -1 from the rank on]."""
        import torch
        n = self.n
        px, rows, ldx, _ = device_block(x, n, None, self.device)
        e, z, info = self._empty((n, n)), (self._empty((n, n)) if null else None), self._empty((n + 1,), torch.int64)
        pe, pi = device_square(e, n, self.device), device_info(info, n, self.device)
        pz = device_square(z, n, self.device) if null else None
        check(lib().blz_rref_device(self.h, C.c_int64(rows), C.c_void_p(px), C.c_int64(ldx), C.c_void_p(pe), C.c_void_p(pz),
                                    C.c_void_p(pi), C.c_void_p(self._stream(stream))))
        return e, z, info

    def set_small(self, which, host):
        check(lib().blz_set_small(self.h, C.c_int(which), ptr(u64(host))))

    def get_small(self, which):
        out = np.zeros(self.n if which == D else self.n * self.n, dtype=np.uint64)
        check(lib().blz_get_small(self.h, C.c_int(which), ptr(out)))
        return out

    def spmv(self, transpose, src, dst):
        check(lib().blz_spmv(self.h, C.c_int(int(transpose)), C.c_int(src), C.c_int(dst)))

    def block_dot(self):
        a = np.zeros(self.n * self.n, dtype=np.uint64)
        b = np.zeros(self.n * self.n, dtype=np.uint64)
        check(lib().blz_block_dot(self.h, ptr(a), ptr(b)))
        return a, b

    def semi_inverse(self):
        npiv = C.c_int(0)
        winv = np.zeros(self.n * self.n, dtype=np.uint64)
        d = np.zeros(self.n, dtype=np.uint64)
        check(lib().blz_semi_inverse(self.h, C.byref(npiv), ptr(winv), ptr(d)))
        return int(npiv.value), winv, d

    def orthogonalize(self):
        check(lib().blz_orthogonalize(self.h))

    def iterate(self, max_iters):
        done, stopped, ms = C.c_int(0), C.c_int(0), C.c_float(0)
        check(lib().blz_iterate(self.h, C.c_int(max_iters), C.byref(done), C.byref(stopped), C.byref(ms)))
        return int(done.value), bool(stopped.value), float(ms.value)

    @property
    def iterations(self):
        return int(lib().blz_iterations(self.h))

    @property
    def p_implicit(self):
        """blz_p_implicit(): 1 while the iteration keeps p as X * E, 0 when the P block holds p itself (test hook)."""
        return int(lib().blz_p_implicit(self.h))

    @property
    def selfdot_active(self):
        """blz_selfdot_active(): 1 when the next iterate() takes both inner products from the products' own outputs."""
        return int(lib().blz_selfdot_active(self.h))

    def set_iterations(self, its):
        check(lib().blz_set_iterations(self.h, C.c_int64(its)))

    def final_check(self):
        a, b = C.c_int(0), C.c_int(0)
        check(lib().blz_final_check(self.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def block_rref(self, block):
        """blz_block_rref(): (E as an n x n array, rank, pivot columns) of the row space of `block`, all ranks merged."""
        E = np.zeros(self.n * self.n, dtype=np.uint64)
        rank = C.c_int(0)
        piv = np.zeros(self.n, dtype=np.int32)
        check(lib().blz_block_rref(self.h, C.c_int(block), ptr(E), C.byref(rank),
                                   piv.ctypes.data_as(C.POINTER(C.c_int32))))
        return E.reshape(self.n, self.n), int(rank.value), [int(q) for q in piv[:rank.value]]

    def kernel_basis(self):
        """blz_kernel_basis(): (k, z as an n x n array); V then holds the k basis vectors in its first k columns."""
        k = C.c_int(0)
        z = np.zeros(self.n * self.n, dtype=np.uint64)
        check(lib().blz_kernel_basis(self.h, C.byref(k), ptr(z)))
        return int(k.value), z.reshape(self.n, self.n)

    def time_kernel(self, which, reps):
        ms = C.c_float(0)
        check(lib().blz_time_kernel(self.h, C.c_int(which), C.c_int(reps), C.byref(ms)))
        return float(ms.value)

    PROFILE_CLASSES = ("spmv1", "spmv2", "block_dot", "semi_inverse", "orthogonalize", "allgather_v",
                       "allgather_tmp", "allreduce", "reduce_scatter")

    def profile(self, enable):
        check(lib().blz_profile(self.h, C.c_int(int(enable))))

    def profile_read(self):
        ms = (C.c_double * len(self.PROFILE_CLASSES))()
        cnt = (C.c_int64 * len(self.PROFILE_CLASSES))()
        check(lib().blz_profile_read(self.h, ms, cnt))
        return {k: dict(ms_total=float(ms[i]), launches=int(cnt[i])) for i, k in enumerate(self.PROFILE_CLASSES)}

    def set_exchange_mode(self, external):
        check(lib().blz_set_exchange_mode(self.h, C.c_int(int(external))))

    def snapshot_begin(self):
        check(lib().blz_snapshot_begin(self.h))

    def snapshot_wait(self, v=None, p=None):
        """(v, p, iterations) of the snapshot; this rank's rows are written into v / p (allocated zero if not given)."""
        n = self.n
        if v is None:
            v = np.zeros(self.rows(V) * n, dtype=np.uint64)
        if p is None:
            p = np.zeros(self.rows(V) * n, dtype=np.uint64)
        its = C.c_int64(0)
        check(lib().blz_snapshot_wait(self.h, ptr(v), ptr(p), C.byref(its)))
        return v, p, int(its.value)

    def sync(self):
        check(lib().blz_sync(self.h))

    def comm_init(self, uid, rank, nranks):
        buf = (C.c_char * len(uid)).from_buffer_copy(uid)
        check(lib().blz_comm_init(self.h, buf, C.c_size_t(len(uid)), C.c_int(rank), C.c_int(nranks)))


def comm_unique_id():
    buf = (C.c_char * 128)()
    check(lib().blz_comm_unique_id(buf, C.c_size_t(128)))
    return bytes(buf)


def solve_rhs(M, b, prime, n, right=False, batch=16, device=0, signed=False, wide=False):
    """M x = b (right) / x M = b on one GPU: dict(status, x, iterations, final_check).
    signed=True: M.x holds int32 bit patterns (signed value mode).
    wide: the wide value mode comes from the matrix (M.x_hi, handed over by set_matrix_rhs); the argument only says so at
    the call site and changes nothing -- a matrix whose residues all fit 32 bits has x_hi None and is an ordinary one."""
    with Context(prime, n, device) as ctx:
        if signed:
            ctx.set_values_signed()
        ctx.set_matrix_rhs(M, b, right)
        ctx.init_v()
        while not ctx.iterate(batch)[1]:
            pass
        fc = ctx.final_check()
        status, x = ctx.solution()
        return dict(status=status, x=x, iterations=ctx.iterations, final_check=fc)


def solve_rhs_device(t_or_triplets, b, prime, n, right=False, batch=16, device=0, reorder=False):
    """M X = B (right) / X M = B with nothing tall on the host: M a 2-D torch sparse COO tensor or a tuple (i, j, x[, nrows,
    ncols]) of device triplets (Context.set_matrix_device), b a (rows,) or (rows, k) tensor on the same GPU (device_rhs()).
    Returns dict(status, x, iterations, final_check): status the list of k statuses of solution_block(), x a (length, k)
    torch.uint64 tensor on the GPU.  reorder=True: the matrix is renumbered on the GPU before the build (the result is the same)."""
    with Context(prime, n, device) as ctx:
        if isinstance(t_or_triplets, (tuple, list)):
            i, j, x, *dims = t_or_triplets
            nrows, ncols = (list(dims) + [None, None])[:2]
        else:
            t = t_or_triplets
            if len(tuple(t.shape)) != 2:
                raise ValueError(f"solve_rhs_device: {len(tuple(t.shape))} dimensions, a matrix has 2")
            idx = t._indices().contiguous()
            i, j, x, nrows, ncols = idx[0], idx[1], t._values().contiguous(), int(t.shape[0]), int(t.shape[1])
        ctx.set_matrix_rhs_device(i, j, x, b, nrows, ncols, right, reorder=reorder)
        ctx.init_v()
        while not ctx.iterate(batch)[1]:
            pass
        fc = ctx.final_check()
        status, xs = ctx.solution_device()
        return dict(status=status, x=xs, iterations=ctx.iterations, final_check=fc)


def solve(M, prime, n, right=False, stop_after=-1, batch=16, device=0, basis=False, signed=False, wide=False,
          device_build=False, device_reorder=False):
    """block_lanczos(), sequential/lanczos_modp.c:585-669, on one GPU.  Returns dict(v, tmp, iterations).
    basis=True (not with stop_after): also reduce the final block to independent kernel vectors (blz_kernel_basis) --
    adds basis (rows x k array), k and z to the result; v, tmp and p stay those of the plain solve.
    signed=True: M.x holds int32 bit patterns (Matrix.load_signed) and an entry a means a mod p.
    wide: the wide value mode comes from the matrix (M.x_hi, handed over by set_matrix); the argument only says so at the
    call site and changes nothing -- a matrix whose residues all fit 32 bits has x_hi None and is an ordinary one.
    device_build=True: the matrix is set with set_matrix_upload (both CSRs built on the GPU, the file's numbering kept; not
    with signed or wide entries); every block of the result is the same, word for word.
    device_reorder=True (with device_build): set_matrix_upload(reorder=True), the numbering made on the GPU; the same result."""
    if basis and stop_after > 0:
        raise ValueError("basis=True needs a run to the end (stop_after < 0)")
    if device_reorder and not device_build:
        raise ValueError("device_reorder=True needs device_build=True")
    if device_build and (signed or getattr(M, "x_hi", None) is not None):
        raise ValueError("device_build=True takes neither signed nor wide entries")
    with Context(prime, n, device) as ctx:
        if signed:
            ctx.set_values_signed()
        if device_build:
            ctx.set_matrix_upload(M, right, reorder=device_reorder)
        else:
            ctx.set_matrix(M, right)
        ctx.init_v()
        while True:
            todo = batch
            if stop_after > 0:
                todo = min(batch, stop_after - ctx.iterations)
                if todo <= 0:
                    break
            _, stopped, _ = ctx.iterate(todo)
            if stopped:
                break
        out = dict(v=ctx.get_block(V), tmp=ctx.get_block(TMP), p=ctx.get_block(P), iterations=ctx.iterations,
                   final_check=ctx.final_check())
        if basis:
            k, z = ctx.kernel_basis()
            out.update(k=k, z=z, basis=ctx.get_block(V).reshape(-1, n)[:, :k].copy())
        return out
