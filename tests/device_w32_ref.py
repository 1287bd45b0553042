"""What the 32-bit device-block launchers choose, restated in plain Python (csrc/blz_devw32.hip), and the case list that
tests/test_gpu_device_w32.py runs.  tests/test_host_device_w32.py checks, without a GPU, that the list reaches every form of
every kernel; the GPU file runs exactly this list.

A block of a case is (n, pad, off): width n, row stride n + pad words, starting `off` 32-bit words into a tensor whose base
is aligned to 16 bytes or more (torch's allocations are), so its pointer is 4 * off mod 16.
"""

TILE_WORDS = 2048                                       # W32_TILE_WORDS: u32 words of one block's LDS tile
BLOCK = 256
MAX_TERMS = 4
PRIMES = (2, 3, 65537, (1 << 30) - 35, (1 << 31) - 1, (1 << 32) - 5)
PIDS = ("p2", "p3", "p16", "p30", "p31", "p32")
WIDTHS = (1, 2, 3, 5, 8, 16, 17, 33, 64)


def log2_ceil(v):
    lg = 0
    while (1 << lg) < v:
        lg += 1
    return lg


def width(ptr_mod16, ld, n):
    """dev_w32_width(): 32-bit words per lane access -- pointer, stride and width must all allow it"""
    if n % 4 == 0 and ld % 4 == 0 and ptr_mod16 % 16 == 0:
        return 4
    if n % 2 == 0 and ld % 2 == 0 and ptr_mod16 % 8 == 0:
        return 2
    return 1


def block_width(n, pad, off):
    return width((4 * off) % 16, n + pad, n)


def call_width(n, blocks):
    """a call runs at the least width of its blocks; blocks: (pad, off) pairs"""
    return min(block_width(n, pad, off) for pad, off in blocks)


def tile_rows(n):
    """dev_w32_tile_rows(): rows of a tile of the inner products"""
    return TILE_WORDS >> log2_ceil(n)


def thread_tile(n):
    """TT: a thread of k_w32_dot owns a TT x TT tile of C"""
    return 1 if n == 1 else 2 if n <= 16 else 4


def dot_form(n, blocks):
    """(TT, V) of k_w32_dot"""
    return thread_tile(n), call_width(n, blocks)


def dot_slices(n):
    tpr = (1 << log2_ceil(n)) // thread_tile(n)
    return BLOCK // (tpr * tpr)


def dot_max_blocks(n, num_cu):
    """dev_dot_max_blocks(): the grid's cap and the partial rows of the scratch, one panel or two"""
    return max(1, min((8 << 20) // (n * n * 8), num_cu * 4))


def combine_shape(n, nterms, nz):
    """(LDS bytes, threads of a workgroup, workgroups a CU is given) of k_w32_combine"""
    lds = nz * nterms * n * n * 4
    if lds <= 40 * 1024:
        return lds, BLOCK, 8
    return lds, 1024, 2 if 2 * lds <= 160 * 1024 else 1


ALL_DOT_FORMS = {(1, 1)} | {(tt, v) for tt in (2, 4) for v in (1, 2, 4)}
ALL_VECTOR_FORMS = {1, 2, 4}

# ---- the case list of the GPU tests

# (pad of x, off of x, pad of y, off of y): strides n .. n + 4, mixed strides, blocks 1, 2 and 3 words into their tensor
DOT_LAYOUTS = ((0, 0, 0, 0), (1, 0, 1, 0), (2, 0, 2, 0), (3, 0, 3, 0), (4, 0, 4, 0), (0, 0, 3, 0), (4, 0, 2, 0),
               (0, 1, 0, 1), (0, 2, 0, 2), (0, 3, 0, 3), (4, 0, 4, 2), (2, 2, 2, 2))
# per term (pad, off); the output takes the first term's layout when in place, COMBINE_OUT otherwise
COMBINE_LAYOUTS = (((0, 0), (0, 0), (0, 0), (0, 0)), ((4, 0), (4, 0), (4, 0), (4, 0)), ((2, 0), (2, 2), (0, 2), (4, 2)),
                   ((0, 0), (3, 0), (2, 0), (1, 0)), ((0, 1), (4, 0), (0, 3), (2, 0)))
COMBINE_OUT = {0: (0, 0), 1: (4, 0), 2: (2, 2), 3: (3, 0), 4: (0, 0)}
IO_LAYOUTS = ((0, 0), (4, 0), (2, 0), (2, 2), (1, 0), (0, 1), (0, 3))
ALIASES = ("abc", "aac", "aba", "abb", "aaa")           # dot_pair32: which of x0, x1, y are one block (a, b, c)


def pair_layout(px, ox, py, oy):
    """(pad, off) of the three blocks a, b, c a dot_pair32 case makes out of one entry of DOT_LAYOUTS"""
    return {"a": (px, ox), "b": (py, oy), "c": (px, oy)}


def dot_rows(n, num_cu=256):
    """rows 0, 1, 2, 63; one short of the tile, the tile, one past it; and every workgroup two tiles with a ragged last one"""
    tr = tile_rows(n)
    return (0, 1, 2, 63, tr - 1, tr, tr + 1), 2 * dot_max_blocks(n, num_cu) * tr + tr // 2 + 1


def dot_forms_reached(pair=False):
    """dot32: x at (px, ox), y at (py, oy).  dot_pair32: x0, x1, y = the blocks of pair_layout() that the pattern names"""
    got = set()
    for n in WIDTHS:
        for lay in DOT_LAYOUTS:
            if not pair:
                got.add(dot_form(n, [lay[:2], lay[2:]]))
                continue
            blk = pair_layout(*lay)
            for pat in ALIASES:
                got.add(dot_form(n, [blk[ch] for ch in pat]))
    return got


def combine_forms_reached(nz):
    got = set()
    for n in WIDTHS:
        for k, lay in enumerate(COMBINE_LAYOUTS):
            for nterms in range(1, MAX_TERMS + 1):
                blocks = list(lay[:nterms]) + [COMBINE_OUT[k]] * nz
                got.add(call_width(n, blocks))
                got.add(call_width(n, list(lay[:nterms])))      # in place: the outputs are terms
    return got


def io_width(n, pad, off):
    """import / export: the slab's rows are padded to a power of two, and a vector form needs the widths to agree"""
    return block_width(n, pad, off) if (1 << log2_ceil(n)) == n else 1


IO_WIDTHS = (8, 5, 4, 2)                                # rand300x200, quirks40x30, the bordered context, the signed one


def io_forms_reached():
    return {io_width(n, pad, off) for n in IO_WIDTHS for pad, off in IO_LAYOUTS}
