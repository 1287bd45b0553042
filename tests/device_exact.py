"""What the launchers of the device block algebra decide, restated on plain integers, and the case lists of
tests/test_gpu_device_exact.py.  Not a test module: test_device_exact_host.py holds the restatement to the bounds of
csrc/modp.h and the case lists to the table of forms, test_gpu_device_exact.py runs the cases.  Nothing here needs a GPU,
torch or the library.

    reduce_model, sum_model      reduce128<0> and the `++cnt == chunk` loop of the kernels (csrc/modp.h)
    dot_shape ... dot_form       launch_dev_dot, dev_dot_max_blocks, k_dev_dot (csrc/blz_devalg.hip)
    dot2_fused, dot2_form        dot_pair_fused, launch_dev_dot at nx = 2 (csrc/blz_devalg.hip)
    combine_form                 launch_dev_combine at nz = 1 (csrc/blz_devalg.hip)
    combine2_form                launch_dev_combine at nz = 2: combine2, combine_shape (csrc/blz_devalg.hip)
    chain_threads, rref_group    launch_dev_chain, group_of (csrc/blz_devsmall.hip)
"""
import itertools
from collections import namedtuple

import exact_ref as X

M64 = (1 << 64) - 1

# ------------------------------------------------------------------------------------------------ primes

P2, P3, P16, P31 = 2, 3, 65537, X.P31
P61, P61B, P62 = X.P61, (1 << 61) - 31, (1 << 62) - 57
TODAY = (P2, P3, P16, P31, P61, P61B, P62)          # the list of the three tests/test_gpu_device_*.py files
P32, P48, P56, P57, P58, P59, P60 = (X.largest_prime_below(1 << k) for k in (32, 48, 56, 57, 58, 59, 60))
P32B = (1 << 32) + 15                               # the first prime of 8-byte words: k = 33
NEW_PRIMES = (P32, P32B, P48, P56, P57, P58, P59, P60)
DEV_PRIMES = NEW_PRIMES + TODAY
_LADDER = X.ladder()
assert all(p in _LADDER for p in DEV_PRIMES if p > 3), [p for p in DEV_PRIMES if p > 3 and p not in _LADDER]
assert (P32, P57, P58, P60) == ((1 << 32) - 5, (1 << 57) - 13, (1 << 58) - 27, (1 << 60) - 93)
assert P61B == X.largest_prime_below(P61) and P62 == X.largest_prime_below(1 << 62)


def barrett(p):
    """p takes the Barrett path with ModP::chunk (launch_dev_*: not `narrow`, c.mers != 61)"""
    return p >= 1 << 32 and p != P61


def acc_class(p):
    """the accumulator and reducer of the dot and combine kernels: `narrow` (p < 2^32: AccS, chunk ignored, whichever
    reducer), c.mers == 61, or Barrett"""
    return "AccS" if p < 1 << 32 else ("fold61" if p == P61 else "Barrett")


def pid(p):
    k = p.bit_length()
    return {P61: "p61f", P61B: "p61b", P32B: "p33"}.get(p, f"p{k}")


# ------------------------------------------------------------------------------------------------ the reducer


def reduce_model(T, p):
    """reduce128<0>(hi, lo, m) of csrc/modp.h on Python integers, with make_modp's mu: floor(2^(63+k) / p) saturated to 64
    bits, th = floor(T / 2^(k-1)) truncated to 64 bits, q = floor(th * mu / 2^64), r = lo - q * p mod 2^64, then p is
    subtracted while r >= p.  Equal to T % p for T < 2^(63+k); past that bound it is whatever the 64-bit words give."""
    assert 0 <= T < 1 << 128
    k = p.bit_length()
    mu = min((1 << (63 + k)) // p, M64)
    hi, lo = T >> 64, T & M64
    sh = k - 1
    th = (((hi << (64 - sh)) & M64) | (lo >> sh)) if sh else lo
    q = (th * mu) >> 64
    r = (lo - q * p) & M64
    return r % p                                    # (the loop of subtractions ends there)


def sum_model(count, p, limit, start=0, term=None):
    """the chunk loop of k_dev_dot / k_dev_combine / k_dev_rref on one accumulator: `count` products of (p-1)^2 (or `term`)
    are added to acc = start, and whenever `limit` of them have gone in since the last reduction, acc <- reduce_model(acc);
    one reduction at the end.  limit = chunk(p) is the kernel; limit = chunk(p) + 1 is the kernel with an off-by-one."""
    term = (p - 1) ** 2 if term is None else term
    acc, cnt = start, 0
    for _ in range(count):
        acc = (acc + term) & ((1 << 128) - 1)
        cnt += 1
        if cnt == limit:
            acc, cnt = reduce_model(acc, p), 0
    return reduce_model(acc, p)


# ------------------------------------------------------------------------------------------------ k_dev_dot (NX = 1, 2)


def log2_ceil(v):
    lg = 0
    while (1 << lg) < v:
        lg += 1
    return lg


def dot_shape(n, cus):
    """(TR, max_blocks, slices, NP, TT): the rows of a tile (TILE_WORDS >> lg), dev_dot_max_blocks (8 MB of scratch or four
    workgroups a CU), and of k_dev_dot the slices a tile's rows are split over, the entries of C per thread and the side of
    a thread's tile of C (launch_dev_dot: np from n * n against BLOCK; dot_np: TT = 1 at n = 1)."""
    lg = log2_ceil(n)
    TR = 1024 >> lg
    max_blocks = max(1, min((8 << 20) // (n * n * 8), cus * 4))
    NP = 1 if n * n <= 256 else (4 if n * n <= 1024 else 16)
    TT = 2 if NP == 1 and n > 1 else 1
    tpr = (1 << lg) // TT
    slices = 256 // (tpr * tpr) if NP == 1 else 1
    return TR, max_blocks, slices, NP, TT


def dot_products_per_accumulator(rows, n, cus):
    """the fewest products one accumulator of the launch takes (0 where a workgroup or a slice gets no row): tile t goes to
    workgroup t mod grid, row r of a tile to slice r mod slices (the loops of k_dev_dot)"""
    TR, max_blocks, slices, _, _ = dot_shape(n, cus)
    ntiles = -(-rows // TR)
    grid = min(ntiles, max_blocks)
    if grid == 0:
        return 0
    least = None
    for b in range(grid):
        mine = range(b, ntiles, grid)
        full = len(mine) - (1 if mine[-1] == ntiles - 1 else 0)
        last = rows - (ntiles - 1) * TR if mine[-1] == ntiles - 1 else 0
        for s in (0, slices - 1):                   # the counts fall with the slice: the first and the last decide
            got = full * len(range(s, TR, slices)) + len(range(s, last, slices))
            least = got if least is None else min(least, got)
    return least


def dot_tiles_past_chunk(p, n, cus):
    TR, _, slices, _, _ = dot_shape(n, cus)
    return -(-(X.chunk(p) + 2) // (TR // slices))


def dot_rows_past_chunk(p, n, cus):
    """T * max_blocks * TR + 1 with T = ceil((chunk + 2) / (TR / slices)): the fewest rows at which every accumulator of
    the launch takes at least chunk + 2 products (T full tiles for every workgroup; the odd row makes one partial tile)"""
    TR, max_blocks, _, _, _ = dot_shape(n, cus)
    return dot_tiles_past_chunk(p, n, cus) * max_blocks * TR + 1


def pair_ok(n, pad):
    """16-byte lane accesses (pair_ok of csrc/blz_devalg.hip) for a torch allocation, which is 16-byte aligned: even width and stride"""
    return n % 2 == 0 and (n + pad) % 2 == 0


DotForm = namedtuple("DotForm", "acc shape lanes")


def dot_form(p, n, vec2):
    """the instantiation of k_dev_dot: accumulator class, 'TT=1' | 'TT=2' | 'NP=4' | 'NP=16', 16- or 8-byte lanes"""
    _, _, _, NP, TT = dot_shape(n, 1)
    return DotForm(acc_class(p), f"TT={TT}" if NP == 1 else f"NP={NP}", 16 if vec2 and n % 2 == 0 else 8)


def dot2_fused(p, n):
    """dot_pair_fused: one k_dev_dot<..., NX = 2> launch, or (Barrett at n > 32) the nx = 1 form twice"""
    return n <= 32 or p < 1 << 32 or p == P61


def dot2_form(p, n, vec2):
    f = dot_form(p, n, vec2)
    return f if dot2_fused(p, n) else f._replace(shape="two dot launches")


# ------------------------------------------------------------------------------------------------ the combines

CombineForm = namedtuple("CombineForm", "acc threads lg")
Combine2Form = namedtuple("Combine2Form", "acc threads lg in_lds dropped_vec2")


def combine_form(p, n, nterms, vec2):
    """launch_dev_combine at nz = 1: 1024 threads where the coefficient matrices take more than 40 KB of LDS, lane groups of
    2^lg lanes, lg from n / 2 in the 16-byte lane form"""
    v2 = vec2 and n % 2 == 0
    threads = 1024 if nterms * n * n * 8 > 40 * 1024 else 256
    return CombineForm(acc_class(p), threads, log2_ceil(n // 2 if v2 else n))


def combine2_form(p, n, masks, vec2):
    """launch_dev_combine at nz = 2: a term's panels go into LDS together while they fit 160 KB (in_lds[t]), else the term reads
    them from global memory; 1024 threads past 40 KB of LDS; k_dev_combine2 has no 1024-thread 16-byte lane form for the
    128-bit accumulators, so that launch drops the lanes (dropped_vec2)"""
    v2 = vec2 and n % 2 == 0
    room, used, in_lds = (160 * 1024) // (n * n * 8), 0, []
    for m in masks:
        need = int(bool(m[0])) + int(bool(m[1]))
        assert need
        in_lds.append(used + need <= room)
        if in_lds[-1]:
            used += need
    threads = 1024 if used * n * n * 8 > 40 * 1024 else 256
    dropped = v2 and threads == 1024 and p >= 1 << 32
    if dropped:
        v2 = False
    return Combine2Form(acc_class(p), threads, log2_ceil(n // 2 if v2 else n), tuple(in_lds), dropped)


def combine2_runs(chunk, n, nterms):
    """the runs combine2_term cuts the nterms * n products of an accumulator into, as (length, reduced before it): a run is
    what is left of the term's row or what the count has room for, chunk - cnt, and the reduction comes when the count is
    full.  A run of length L is L // 2 turns of the two-word loop and, if L is odd, the single trailing product."""
    runs, cnt = [], 0
    for _ in range(nterms):
        i = 0
        while i < n:
            reduced = cnt == chunk
            if reduced:
                cnt = 0
            run = min(n - i, chunk - cnt)
            assert run > 0
            cnt, i = cnt + run, i + run
            runs.append((run, reduced))
    return runs


ALL_MASKS = [m for k in range(1, 5) for m in itertools.product(((1, 1), (1, 0), (0, 1)), repeat=k)
             if any(a for a, _ in m) and any(b for _, b in m)]


# ------------------------------------------------------------------------------------------------ the small algebra


def chain_threads(n):
    """launch_dev_chain: (threads, lg) -- G x G threads, G the power of two >= n, between 64 and 1024"""
    lg = log2_ceil(n)
    return min(1024, max(64, 1 << (2 * lg))), lg


def rref_group(n):
    """group_of: the lanes of a row of k_dev_rref"""
    return 1 << log2_ceil(n)


def rref_tile_rows(n):
    """rows of a k_dev_rref tile: 4 wavefronts, DEVRREF_U = 8 rows per lane group"""
    return 4 * 8 * (64 // rref_group(n))


def rref_tiles(n):
    """tiles per workgroup of the echelon block of test_rref_where_the_reduction_is_longest: the n - 1 echelon rows in tiles
    of rref_tile_rows(n), then a tile of sum rows -- two where a tile holds the echelon (n <= 33), three at n = 48 and 64"""
    return max(-(-(n - 1) // rref_tile_rows(n)), 1) + 1


def rref_rows(n, cus):
    """rref_tiles(n) tiles for each of the 2 * CUs workgroups of the partial pass (partial_blocks), and five rows"""
    return rref_tiles(n) * (2 * cus) * rref_tile_rows(n) + 5


# ------------------------------------------------------------------------------------------------ the cases of the GPU file

FULL = (P57, P61)                                   # every width at the tight 57-bit prime and at the folding one
OTHER_NEW = tuple(p for p in NEW_PRIMES if p not in FULL)
FULL_WIDTHS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 33, 48, 63, 64)
OTHER_WIDTHS = (2, 8, 24, 64)
PADS = (0, 2, 3)                                    # strides n, n + 2, n + 3; the mixed calls take one of each

# A. random residues.  (P32, 32): where k_dev_combine2 keeps the 16-byte lanes in a 1024-thread launch with lane groups of 16
# (eight panels of 8 KB, the 96-bit accumulators); (P32, 33): that class with lane groups of 64 in a 256-thread launch
RANDOM_CASES = [(p, n) for p in FULL for n in FULL_WIDTHS] + [(p, n) for p in OTHER_NEW for n in OTHER_WIDTHS]
COMBINE_EXTRA = [(P32, 32), (P32, 33)]
MASKS = {1: [((1, 1),)],                            # those of test_gpu_device_fused.py (the GPU file holds them equal)
         2: [((1, 0), (0, 1)), ((1, 1), (0, 1))],
         3: [((1, 0), (1, 1), (1, 1))],
         4: [((1, 1), (0, 1), (1, 0), (1, 1)), ((1, 1), (1, 1), (1, 1), (1, 1))]}
WIDE_MASKS = [((1, 0), (1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1), (1, 1)), ((1, 1), (1, 1), (0, 1), (1, 0))]
COMBINE_PADS = ((0,), (2,), (3,), (0, 3, 2, 1))


DOT_EXTRA = [(P32, 1)]                              # the 96-bit accumulators at n = 1 (TT = 1)
DOT_PADS = ((0, 0, 0), (2, 2, 2), (3, 3, 3), (3, 0, 2))        # the strides of x0, x1 and y (dot: of x and y, the outer two)


def dot_rows(n):
    TR = dot_shape(n, 1)[0]
    return (1, TR - 1, TR + 1, 2 * TR + 3)


def combine_plan(n):
    """(number of terms, the terms' paddings in turn) of every combine case at width n"""
    return [(k, pads) for k in combine_terms(n) for pads in COMBINE_PADS]


def pair_plan(n):
    """(masks, the terms' paddings in turn) of every combine_pair case at width n"""
    return [(m, pads) for m in pair_masks(n) for pads in COMBINE_PADS]


def lanes16(n, pads, nterms):
    """every term of the call allows 16-byte lanes (the outputs of the call are new blocks of stride n, or terms)"""
    return all(pair_ok(n, pads[t % len(pads)]) for t in range(nterms))


def combine_rows(n):
    """1, 63 and 257 rows, and 70 from n = 33 on (the row count of tests/test_gpu_device_algebra.py at n = 64)"""
    return (1, 63, 257) if n <= 32 else (1, 63, 70, 257)


def combine_terms(n):
    """1 ... 4 terms at every width: at n = 48 two terms are the 256-thread launch and three the 1024-thread one"""
    return (1, 2, 3, 4)


def pair_masks(n):
    """the MASKS of the fused file; from n = 33 on also the panel counts that fill and overflow the LDS at n = 64"""
    out = [m for k in (1, 2, 3, 4) for m in MASKS[k]]
    return out + [m for m in WIDE_MASKS if m not in out] if n >= 33 else out


# B. dots past the chunk
PAST_PRIMES = (P57, P58, P59, P60, P62, P61B, P61)
PAST_WIDTHS = (1, 4, 8, 16, 24, 64)
PAST_CUS = (8, 256, 304)
DOT_PAST = [(p, n) for p in PAST_PRIMES for n in PAST_WIDTHS]

# C. combines past the chunk: (p, n, terms) with terms * n >= chunk + 2
COMBINE_PAST = [(P57, 32, 3), (P57, 48, 2), (P57, 64, 2), (P57, 64, 4),
                (P58, 12, 3), (P58, 16, 3), (P58, 33, 1),
                (P59, 8, 3), (P59, 6, 3), (P59, 5, 4),
                (P60, 5, 2), (P60, 6, 2), (P60, 9, 1),
                (P61B, 5, 2), (P61B, 6, 2), (P61B, 8, 1),
                (P62, 5, 2), (P62, 6, 2), (P62, 1, 3), (P62, 3, 1),
                (P61, 24, 2), (P61, 64, 3), (P61, 12, 3)]


def past_masks(terms):
    """which outputs the terms of a past-the-chunk combine_pair enter: the first term enters z0 only, so the runs of the
    second start in the middle of the count; with one term it enters both"""
    return ((1, 1),) if terms == 1 else ((1, 0),) + ((1, 1),) * (terms - 1)


# D. small algebra
SMALL_CASES = [(p, n) for p in FULL for n in (2, 4, 12, 24, 32, 33, 48, 63)] + [(p, n) for p in OTHER_NEW for n in (8, 24, 64)]
RREF_PAST = [(P58, 48), (P58, 64), (P59, 24), (P59, 32), (P60, 12), (P60, 16), (P61B, 8), (P62, 4), (P62, 24)]
RREF_VALUES = [(P57, 24), (P57, 64), (P57, 1), (P57, 2), (P61, 2), (P61, 33)]     # no width passes the chunk at these
RREF_CASES = RREF_PAST + RREF_VALUES
CHAIN_PAST = RREF_PAST                              # n >= chunk + 2 as well: the n products of a word of W * S in k_dev_chain
RREF_RANDOM = [(p, n) for p in FULL for n in FULL_WIDTHS]


def rref_random_rows(n):
    """one row, two more rows than columns, and two tiles and three rows"""
    return (1, n + 2, 2 * rref_tile_rows(n) + 3)


# E. one rebuilt iteration per new class
ITER_CASES = [(24, P57), (32, P58), (12, P60), (2, P32B), (4, P32)]
