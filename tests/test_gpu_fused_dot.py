"""The fused inner products -- v^T Av and Av^T Av as the epilogue of the second SpMV of an iteration -- against exact
integers, in every form the epilogue exists in: k_spmv_dot, k_spmv_staged<DOT>, k_spmv_panel<DOT>, k_spmv_wave<DOT>,
k_spmv_heavy<DOT> and k_spmv_heavy_combine<DOT>.

The expectation is fused_ref's closed form (plain Python integers; tests/test_fused_ref.py holds it against exact_ref
and the oracle): every block row of v is p - 1 - k ("ramp") or p - 1 ("max"), so every word of v and Av is within
2^-16 of p and every entry of the two n x n matrices is a different multiple of sum_c s_c resp. sum_c s_c^2.

Every case reads the slab's plan (Context.plan, blz_slab_plan) after set_matrix and asserts the form, the lists and the
grids it was written for: a case that does not reach its kernel fails.  "Past chunk" cases size the matrix from the plan's
grids so that every accumulator of the launch (a lane group of the streaming launch, a wavefront of k_spmv_wave, a
workgroup of k_spmv_heavy, a lane group of the combine launch) takes at least chunk + 2 rows: at the 57- to 62-bit Barrett
primes one product more than make_modp allows in a sum is then a wrong word (test_fused_ref.py:
test_one_product_too_many_of_these_words_overflows_the_reducer).  "Exact totals" cases run both operands and both
orientations on matrices whose rows go to all the launches at once.

After one iterate(1): VTAV, VTAAV, the whole of TMP and AV against the closed form, V and P against the oracle's update
fed the device's own winv and d.  No tolerance: equality of u64 words.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import blz
import exact_ref as X
import fused_ref as F
import oracle as orc

pytestmark = pytest.mark.gpu

P61 = X.P61
P57 = X.largest_prime_below(1 << 57)
P62 = X.largest_prime_below(1 << 62)
P61B = X.largest_prime_below(P61)
P60 = X.largest_prime_below(1 << 60)
FULL = (P57, P61)
EDGE = tuple(X.largest_prime_below(1 << k) for k in (58, 59, 60)) + (P61B, P62)      # as in test_gpu_exact.py
PRIMES = FULL + EDGE
SEG = 4096                      # entries per segment of k_spmv_heavy (HEAVY_SEG)
TAIL_NNZ = 4000000              # below this many entries a slab runs the TAILB = true instantiation


def pid(p):
    return f"p{p.bit_length()}{'f' if p == P61 else ''}"


def pow2(n):
    w = 1
    while w < n:
        w <<= 1
    return w


_CUS = []


def cus():
    """Compute units the library sizes its grids by (from the plan of a tiny matrix)."""
    if not _CUS:
        with blz.Context(65537, 1) as c:
            c.set_matrix(blz.Matrix(2, 2, [0, 1], [0, 1], [1, 1]), False)
            _CUS.append(c.plan(False)["num_cu"])
        assert _CUS[0] > 0
    return _CUS[0]


def pad_rows(n):
    """With at least this many rows no slab shares a row between lane groups (spmv_split_log2 = 0), so the outlier
    threshold is BLZ_HEAVY_THR itself."""
    return 2 * cus() * 8 * (256 // pow2(n)) + 1


def wave_limit(n):
    """Longest row one wavefront of k_spmv_wave takes: 256 entries per lane group."""
    G = pow2(n)
    return 256 * 64 // G if G < 64 else 0


def classify(lengths, thr, n):
    """(rows of k_spmv_wave, segments of k_spmv_heavy, split rows) for rows of these lengths (upload_csr's rule)."""
    L = np.asarray(lengths, dtype=np.int64)
    out = L[L > thr]
    medium = int((out <= wave_limit(n)).sum())
    heavy = out[out > wave_limit(n)]
    segs = -(-heavy // SEG)
    return medium, int(segs.sum()), int((segs > 1).sum())


def to_blz(A, right, p):
    nr, nc, i, j, x = F.as_matrix(A, right)
    return blz.Matrix(nr, nc, i, j, (x % p).astype(np.uint32))


def other_block(rows, n, p):
    """The block P starts from: words near p, different in every column."""
    return np.tile(np.array([(p - 2 - 3 * k) % p for k in range(n)], dtype=np.uint64), rows)


def check_iteration(ctx, A, p, n, right, kinds=("ramp", "max")):
    """init_v, V and P set, one iteration, every result against the closed form."""
    for kind in kinds:
        e = F.expect(A, n, p, kind)
        if p >= 1 << 31:
            assert e["sum_s"] % p and e["sum_s2"] % p, "the iteration would stop before the update"
        pb = other_block(A.nrows, n, p)
        ctx.init_v()
        ctx.set_block(blz.V, e["v"])
        ctx.set_block(blz.P, pb)
        done, stopped, _ = ctx.iterate(1)
        a, b = ctx.get_small(blz.VTAV), ctx.get_small(blz.VTAAV)
        av = ctx.get_block(blz.AV)
        bad = np.flatnonzero(av != e["Av"])
        lens = np.bincount(A.i, minlength=A.nrows)
        assert bad.size == 0, (kind, "AV", bad.size, [(int(r), int(lens[r])) for r in np.unique(bad[:64] // n)[:8]])
        assert np.array_equal(ctx.get_block(blz.TMP), e["tmp"]), (kind, "TMP")
        assert np.array_equal(a, e["vtAv"]), (kind, "vtAv", np.flatnonzero(a != e["vtAv"]).tolist(), a[:3], e["vtAv"][:3])
        assert np.array_equal(b, e["vtAAv"]), (kind, "vtAAv", np.flatnonzero(b != e["vtAAv"]).tolist(), b[:3], e["vtAAv"][:3])
        if p >= 1 << 31:
            assert done == 1 and not stopped
        if stopped:
            wv, wp = e["v"], pb
        else:
            winv, d = ctx.get_small(blz.WINV), ctx.get_small(blz.D)
            wv, wp = orc.orthogonalize(e["v"], pb, d, e["vtAv"], e["vtAAv"], winv, A.nrows, e["Av"], n, p, omp_threads=8)
        assert np.array_equal(ctx.get_block(blz.V), wv), (kind, "V")
        assert np.array_equal(ctx.get_block(blz.P), wp), (kind, "P")


def fused_plan(ctx, right, form, n):
    """The plan of the product that carries the epilogue; asserts that the iteration fuses and which form it takes."""
    pl = ctx.plan(right)
    assert pl["width"] == pow2(n) and pl["chunk"] == X.chunk(ctx.prime) and pl["dot_supported"] == 1
    assert pl["fused"] == 1 and pl["fuse_local_off"] == 0 and pl["pieces"] == 1, pl
    assert pl["dot"]["form"] == form, pl
    first = ctx.plan(not right)
    assert first["fused"] == 0
    return pl


def stream_accumulators(pl):
    """Lane groups of the streaming launch of the fused product."""
    threads = 1024 if pl["dot"]["form"] == "panel" else 256
    return pl["dot"]["grid_stream"] * threads // pl["width"]


def rows_past_chunk(p, accumulators):
    return (X.chunk(p) + 2) * accumulators + 1


def variant(k):
    """(right, operand) number k of the four."""
    return bool(k & 1), ("ramp", "max")[(k >> 1) & 1]


SHORT = (0, 1, 3, 4, 5, 63, 64)         # rows the streaming launch keeps at a threshold of 64

# ------------------------------------------------------------------------------------------------ k_spmv_dot

DOT_CASES = []
for _k, _p in enumerate(PRIMES):
    DOT_CASES.append((_p, 8, True, _k % 2, _k))                 # TAILB = true, XCD ranges off / on in turn
    DOT_CASES.append((_p, 8, False, (_k + 1) % 2, _k + 2))      # TAILB = false, the other setting
for _p in (P57, P62):
    DOT_CASES += [(_p, 8, True, 1 - PRIMES.index(_p) % 2, 1), (_p, 8, False, PRIMES.index(_p) % 2, 3)]
    DOT_CASES += [(_p, _n, None, _n % 2, _n) for _n in (1, 2, 4, 3, 5, 7)]


@pytest.mark.parametrize("p,n,tail,xcd,k", DOT_CASES,
                         ids=[f"{pid(p)}-n{n}-tail{'x' if t is None else int(t)}-xcd{x}-{k % 4}" for p, n, t, x, k in DOT_CASES])
def test_k_spmv_dot_past_chunk_rows_per_lane_group(monkeypatch, p, n, tail, xcd, k):
    """A scattered permutation (and a few rows of 0 ... 64 entries): every row stays in the streaming launch."""
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_NO_STAGE", "1")
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    monkeypatch.setenv("BLZ_XCD_RANGES", str(xcd))
    w = pow2(n)
    rows = rows_past_chunk(p, cus() * (4 if w >= 8 else 6) * (256 // w))
    if tail is False:
        rows = max(rows, TAIL_NNZ + 1)
    elif tail is True:
        assert rows < TAIL_NNZ - 1000
    right, kind = variant(k)
    A = F.mixed([F.perm(rows, seed=k + 1, mode=("ones", "palette", "array")[k % 3]), F.ladder(SHORT, repeat=3, mode="palette")])
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(to_blz(A, right, p), right)
        pl = fused_plan(ctx, right, "spmv", n)
        assert pl["locality"] >= 0.6 and pl["tail_batch"] == (A.nnz < TAIL_NNZ), pl
        if tail is not None:
            assert pl["tail_batch"] == int(tail)
        assert pl["dot"]["xcd_ranges"] == xcd and pl["heavy_thr"] == 64, pl
        assert (pl["n_medium"], pl["n_heavy"], pl["n_multi"]) == (0, 0, 0)
        assert pl["dot"]["grid_heavy"] == pl["dot"]["grid_medium"] == pl["dot"]["grid_combine"] == 0
        assert A.nrows >= rows_past_chunk(p, stream_accumulators(pl)), (A.nrows, pl)
        check_iteration(ctx, A, p, n, right, (kind,))


# ------------------------------------------------------------------------------------------------ k_spmv_staged<DOT>

STAGED_LENGTHS = (1, 1, 1, 3, 4, 5, 1, 1, 1, 60, 1, 1, 1, 2, 1, 1)     # one row in 16 overflows a 64-entry window
STAGED_CASES = [(p, 8, ("64", "4096")[k % 2], k) for k, p in enumerate(PRIMES)] + \
               [(P57, 8, "4096", 1), (P62, 8, "64", 2), (P57, 4, "4096", 3), (P57, 4, "64", 0)]


@pytest.mark.parametrize("p,n,capw,k", STAGED_CASES, ids=[f"{pid(p)}-n{n}-capw{c}-{k % 4}" for p, n, c, k in STAGED_CASES])
def test_k_spmv_staged_dot_past_chunk_rows_per_lane_group(monkeypatch, p, n, capw, k):
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_STAGE_ALWAYS", "1")
    monkeypatch.setenv("BLZ_STAGE_CAPW", capw)
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    w = pow2(n)
    rows = rows_past_chunk(p, cus() * 4 * (256 // w))
    right, kind = variant(k)
    if n == 4 and capw == "64":         # 16 rows per tile: only rows of one entry leave a 64-entry window any room
        A, mode = F.perm(rows, seed=5, mode="palette"), "palette"
    else:
        # (a 4096-entry window holds one stream per wavefront and buffer: ones or the packed palette)
        mode = ("ones", "palette")[k % 2] if capw == "4096" else ("array", "ones", "palette")[k % 3]
        # (n = 4 needs twice the rows: shorter rows keep the columns below 2^24, where the stream still packs)
        lengths = STAGED_LENGTHS if n == 8 else tuple(min(q, 20) for q in STAGED_LENGTHS)
        A = F.ladder(lengths, repeat=-(-rows // len(lengths)), mode=mode, seed=k)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(to_blz(A, right, p), right)
        pl = fused_plan(ctx, right, "staged", n)
        assert pl["st_ok"] == 1 and pl["st_dyn"] == 0 and pl["st_capw"] == int(capw) and pl["dot"]["st_gathers"] == 4, pl
        assert pl["packed"] == (2 if mode == "array" else 1 if mode == "palette" else 0) or n == 4, pl
        assert (pl["n_medium"], pl["n_heavy"]) == (0, 0) and pl["heavy_thr"] == 64
        if capw == "64" and n == 8:     # a tile of st_tr rows with the 60-entry row in it does not fit the window
            assert pl["st_tr"] <= 16 and 60 + pl["st_tr"] - 1 > pl["st_capw"]
        assert A.nrows >= rows_past_chunk(p, stream_accumulators(pl)), (A.nrows, pl)
        check_iteration(ctx, A, p, n, right, (kind,))


# ------------------------------------------------------------------------------------------------ k_spmv_panel<DOT>

PANEL_CASES = [(p, (None, "37")[k % 2], k) for k, p in enumerate(PRIMES)] + [(P57, "37", 3), (P62, None, 0)]


@pytest.mark.parametrize("p,cap,k", PANEL_CASES, ids=[f"{pid(p)}-cap{c}-{k % 4}" for p, c, k in PANEL_CASES])
def test_k_spmv_panel_dot_past_chunk_rows_per_lane_group(monkeypatch, p, cap, k):
    """Every output row reads two of 37 shared operand rows (a third of the entries): the renumbering plans a panel."""
    n = 8
    if cap:
        monkeypatch.setenv("BLZ_PANEL_ROWS", cap)
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    blocks = (cus() + 7) & ~7
    rows = rows_past_chunk(p, blocks * 1024 // n)
    right, kind = variant(k)
    A = F.hot(rows, rows // 2 + 100, 4, 37, mode=("ones", "palette", "array")[k % 3], seed=k)
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(to_blz(A, right, p), right)
        pl = fused_plan(ctx, right, "panel", n)
        assert 0 < pl["panel_rows"] <= (37 if cap else 128 * 1024 // (8 * n)), pl
        if cap:
            assert pl["panel_rows"] == 37 and ctx.panel_rows(right)[1] > 0.3
        assert pl["dot"]["grid_stream"] == blocks and (pl["n_medium"], pl["n_heavy"]) == (0, 0)
        assert A.nrows >= rows_past_chunk(p, stream_accumulators(pl)), (A.nrows, pl)
        check_iteration(ctx, A, p, n, right, (kind,))


# ------------------------------------------------------------------------------------------------ outlier launches


def outlier_env(monkeypatch):
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    monkeypatch.setenv("BLZ_NO_STAGE", "1")
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")


def check_lists(pl, A, n):
    lens = np.bincount(A.i, minlength=A.nrows)
    assert pl["heavy_thr"] == 64, pl
    assert (pl["n_medium"], pl["n_heavy"], pl["n_multi"]) == classify(lens, 64, n), pl
    d = pl["dot"]
    assert d["grid_medium"] == min(-(-pl["n_medium"] // 4), cus() * 6)
    assert d["grid_heavy"] == min(pl["n_heavy"], cus() * 4, pl["max_dot_blocks"] // 4)
    assert d["grid_combine"] == min(-(-pl["n_multi"] // (256 // pl["width"])), 16)
    assert d["grid_stream"] + d["grid_heavy"] + d["grid_combine"] + d["grid_medium"] <= pl["max_dot_blocks"]
    return lens


@pytest.mark.parametrize("p", PRIMES, ids=[pid(p) for p in PRIMES])
def test_k_spmv_wave_dot(monkeypatch, p):
    """Many rows just above the threshold: one wavefront each.  Past chunk + 2 rows per wavefront where chunk <= 7; both
    operands and orientations (exact totals) at every prime."""
    n = 8
    outlier_env(monkeypatch)
    crossing = X.chunk(p) <= 7
    waves = cus() * 6 * 4
    edge = (63, 64, 65, 66, wave_limit(n), wave_limit(n) + 1, 0, 1, 3, 4, 5)

    def matrix(medium):
        return F.mixed([F.ladder((65,), repeat=medium, mode="palette", seed=1), F.ladder(edge, repeat=2, mode="array", seed=2),
                        F.perm(pad_rows(n), seed=3)])

    # (rows of 65 entries, past chunk: one orientation and operand; exact totals: all four)
    runs = [(3001, q, False) for q in range(4)]
    if crossing:
        runs.insert(0, (rows_past_chunk(p, waves), PRIMES.index(p), True))
    A, have = None, 0
    for medium, q, past in runs:
        if medium != have:
            A, have = matrix(medium), medium
        right, kind = variant(q)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(to_blz(A, right, p), right)
            pl = fused_plan(ctx, right, "spmv", n)
            check_lists(pl, A, n)
            assert pl["n_medium"] == medium + 2 * 3 and pl["n_heavy"] == 2 and pl["n_multi"] == 0, pl
            if past:
                assert pl["dot"]["grid_medium"] * 4 == waves
                assert medium >= rows_past_chunk(p, pl["dot"]["grid_medium"] * 4)
            check_iteration(ctx, A, p, n, right, (kind,))


@pytest.mark.parametrize("p", PRIMES, ids=[pid(p) for p in PRIMES])
def test_k_spmv_heavy_and_combine_dot(monkeypatch, p):
    """Rows past the wavefront limit (one segment: k_spmv_heavy finishes them) and past 4096 and 8192 entries (split:
    k_spmv_heavy_combine finishes them).  Past chunk + 2 rows per workgroup resp. lane group at 2^62-57 and the 61-bit
    Barrett prime; both operands and orientations at every prime."""
    n = 8
    outlier_env(monkeypatch)
    crossing = p in (P62, P61B)
    small = F.mixed([F.ladder((wave_limit(n) + 1, SEG, SEG + 1, 2 * SEG + 1, 64, 65, 0, 3), repeat=9, mode="array", seed=4),
                     F.perm(pad_rows(n), seed=3)])
    mats = [small]
    if crossing:
        whole = rows_past_chunk(p, cus() * 4)
        split = rows_past_chunk(p, 16 * (256 // n))
        # in this order, unshuffled: workgroup b of k_spmv_heavy takes segments b, b + grid, ... of the list
        mats.insert(0, F.mixed([F.ladder((wave_limit(n) + 1,), repeat=whole), F.ladder((SEG + 1,), repeat=split),
                                F.perm(pad_rows(n), seed=3)]))
    k = PRIMES.index(p)
    for A, qs in zip(mats, ((k,), (0, 1, 2, 3)) if crossing else ((0, 1, 2, 3),)):
        for q in qs:
            right, kind = variant(q)
            with blz.Context(p, n) as ctx:
                ctx.set_matrix(to_blz(A, right, p), right)
                pl = fused_plan(ctx, right, "spmv", n)
                check_lists(pl, A, n)
                assert pl["n_heavy"] > 0 and pl["n_multi"] > 0 and pl["dot"]["grid_combine"] > 0
                if A is not small:
                    assert pl["n_medium"] == 0 and pl["n_multi"] == split and pl["n_heavy"] == whole + 2 * split
                    assert pl["dot"]["grid_heavy"] == cus() * 4 and pl["dot"]["grid_combine"] == 16
                    # whole rows first in the list: every workgroup meets at least chunk + 2 of them
                    assert whole // pl["dot"]["grid_heavy"] >= X.chunk(p) + 2
                    assert split >= rows_past_chunk(p, pl["dot"]["grid_combine"] * (256 // n))
                check_iteration(ctx, A, p, n, right, (kind,))


# ------------------------------------------------------------------------------------------------ everything at once


def mixed_matrix(n, mode="array", with_hot=False, seed=8):
    """Streaming rows, rows at the threshold, medium rows, one-segment and split rows, in one matrix, rows shuffled."""
    wl = wave_limit(n)
    lengths = (0, 1, 3, 4, 5, 63, 64, 65, 66, 300, wl, wl + 1, SEG, SEG + 1, 2 * SEG + 1, 4 * wl + 1)
    parts = [F.perm(pad_rows(n), seed=3, mode=mode), F.ladder(lengths, repeat=5, mode=mode, seed=2), F.perm(5000, None, mode)]
    if with_hot:
        parts.append(F.hot(60000, 40000, 4, 37, mode=mode, seed=5))
    return F.shuffled_rows(F.mixed(parts), seed=seed)


def check_all_lists_in_use(pl, A, n):
    check_lists(pl, A, n)
    d = pl["dot"]
    assert min(pl["n_medium"], pl["n_heavy"], pl["n_multi"]) > 0, pl
    assert min(d["grid_stream"], d["grid_heavy"], d["grid_combine"], d["grid_medium"]) > 0, pl


@pytest.mark.parametrize("form", ["spmv", "staged", "panel"])
@pytest.mark.parametrize("p,n,mode", [(P57, 8, "array"), (P61, 8, "palette"), (P62, 5, "ones"), (P60, 8, "palette")],
                         ids=lambda v: pid(v) if isinstance(v, int) and v > 64 else str(v))
def test_all_launches_in_one_matrix(monkeypatch, p, n, mode, form):
    """Exact totals with every partial-row slot in use at once: streaming + medium + heavy + split rows."""
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    if form == "panel":
        monkeypatch.setenv("BLZ_PANEL_MIN_PCT", "10")
    else:
        monkeypatch.setenv("BLZ_NO_REORDER", "1")
        monkeypatch.setenv("BLZ_NO_STAGE" if form == "spmv" else "BLZ_STAGE_ALWAYS", "1")
    A = mixed_matrix(n, mode, with_hot=form == "panel")
    for q in range(4):
        right, kind = variant(q)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(to_blz(A, right, p), right)
            pl = fused_plan(ctx, right, form, n)
            if form == "panel":
                assert pl["panel_rows"] > 0
            check_all_lists_in_use(pl, A, n)
            check_iteration(ctx, A, p, n, right, (kind,))


@pytest.mark.parametrize("n", [8, 5])
def test_column_pieces(monkeypatch, n):
    """The products cut into three column pieces: the epilogue rides on the last one, which adds to what the first two
    left in AV (accum = 1); a row can be an outlier in one piece and ordinary in the next."""
    monkeypatch.setenv("BLZ_FORCE_COMM", "1")
    monkeypatch.setenv("BLZ_AG_CHUNKS", "3")
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    p = P57
    A = mixed_matrix(n, "palette")
    for q in range(4):
        right, kind = variant(q)
        with blz.Context(p, n) as ctx:
            ctx.comm_init(blz.comm_unique_id(), 0, 1)
            ctx.set_matrix(to_blz(A, right, p), right, 0, 1)
            plans = [ctx.plan(right, k) for k in range(3)]
            assert [pl["pieces"] for pl in plans] == [3, 3, 3] and [pl["fused"] for pl in plans] == [0, 0, 1], plans
            assert sum(pl["nnz"] for pl in plans) == A.nnz and all(pl["rows"] == plans[0]["rows"] for pl in plans)
            assert sum(pl["n_medium"] + pl["n_heavy"] for pl in plans) > 0
            check_iteration(ctx, A, p, n, right, (kind,))


@pytest.mark.parametrize("p", [(1 << 31) - 1, 4294967291, 65537])
def test_32_bit_words(monkeypatch, p):
    """AccS accumulators: chunk never binds, the totals must be exact."""
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    monkeypatch.setenv("BLZ_NO_REORDER", "1")
    n = 8
    A = mixed_matrix(n, "palette")
    for q in range(4):
        right, kind = variant(q)
        with blz.Context(p, n) as ctx:
            assert ctx.word_bytes == 4
            ctx.set_matrix(to_blz(A, right, p), right)
            pl = ctx.plan(right)
            assert pl["fused"] == 1
            check_all_lists_in_use(pl, A, n)
            check_iteration(ctx, A, p, n, right, (kind,))


def test_a_band_matrix_keeps_the_inner_products_apart():
    """fuse_local_off: gathers that hit at 2^61-1, n = 8 -- the plan says the iteration does not fuse, and the same closed
    form comes out of the staged product plus the matrix-core inner products."""
    p, n = P61, 8
    A = F.band(150000, 20, "palette")        # enough rows that no lane groups share one (else the slab is not staged)
    for q in range(4):
        right, kind = variant(q)
        with blz.Context(p, n) as ctx:
            ctx.set_matrix(to_blz(A, right, p), right)
            pl = ctx.plan(right)
            assert pl["fuse_local_off"] == 1 and pl["fused"] == 0 and pl["dot_supported"] == 1, pl
            assert pl["plain"]["form"] == "staged" and pl["locality"] < 0.3, pl
            check_iteration(ctx, A, p, n, right, (kind,))


# ------------------------------------------------------------------------------------------------ switches

SWITCHES = {
    "default": {},
    "no_side": {"BLZ_NO_SIDE": "1"},
    "heavy_thr_32": {"BLZ_HEAVY_THR": "32"},
    "heavy_thr_300": {"BLZ_HEAVY_THR": "300"},
    "blocks_per_cu_1": {"BLZ_SPMV_BLOCKS_PER_CU": "1"},
    "blocks_per_cu_8": {"BLZ_SPMV_BLOCKS_PER_CU": "8"},
    "stage_u_4": {"BLZ_STAGE_U": "4", "BLZ_STAGE_ALWAYS": "1", "BLZ_NO_PAIR": "1"},
    "stage_u_8": {"BLZ_STAGE_U": "8", "BLZ_STAGE_ALWAYS": "1", "BLZ_NO_PAIR": "1"},
    "stage_interleave": {"BLZ_STAGE_INTERLEAVE": "1", "BLZ_STAGE_ALWAYS": "1"},
    "reorder_plain": {"BLZ_REORDER_PLAIN": "1"},
    "mfma_block": {"BLZ_MFMA_BLOCK": "256", "BLZ_MFMA_MIN_ROWS": "0"},
    "mfma_per_cu": {"BLZ_MFMA_PER_CU": "1", "BLZ_MFMA_MIN_ROWS": "0"},
}


def switch_case(p, n, name):
    """One iteration on the mixed matrix under the switch `name` (the environment is already set)."""
    env = SWITCHES[name]
    thr = int(env.get("BLZ_HEAVY_THR", "64"))
    A = mixed_matrix(n, "palette")
    lens = np.bincount(A.i, minlength=A.nrows)
    right, kind = variant(sorted(SWITCHES).index(name))
    with blz.Context(p, n) as ctx:
        ctx.set_matrix(to_blz(A, right, p), right)
        pl, first = ctx.plan(right), ctx.plan(not right)
        assert pl["fused"] == (1 if n <= 8 else 0) and pl["dot_supported"] == pl["fused"], pl
        assert pl["heavy_thr"] == thr and (pl["n_medium"], pl["n_heavy"], pl["n_multi"]) == classify(lens, thr, n), pl
        assert min(pl["n_medium"], pl["n_heavy"], pl["n_multi"]) > 0
        if "BLZ_SPMV_BLOCKS_PER_CU" in env:
            per = int(env["BLZ_SPMV_BLOCKS_PER_CU"])
            for q in (first, pl):
                if q["plain"]["form"] == "staged":
                    assert q["st_per_cu"] == per, q
                if q["plain"]["form"] != "panel":
                    assert q["plain"]["grid_stream"] <= ((cus() * per + 7) & ~7), q
            if first["plain"]["form"] == "spmv":
                assert first["plain"]["grid_stream"] >= cus() * per, first
        if "BLZ_STAGE_U" in env:
            assert first["plain"]["form"] == "staged" and first["plain"]["st_gathers"] == int(env["BLZ_STAGE_U"]), first
            assert pl["dot" if n <= 8 else "plain"]["form"] == "staged"
            if n <= 8:
                assert pl["dot"]["st_gathers"] == 4         # the fused form keeps four gathers in flight
        if "BLZ_STAGE_INTERLEAVE" in env:
            assert pl["st_interleave"] == 1 and first["st_interleave"] == 1 and first["plain"]["form"] == "staged"
        check_iteration(ctx, A, p, n, right, (kind,))


@pytest.mark.parametrize("name", sorted(SWITCHES))
@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("p", FULL, ids=[pid(p) for p in FULL])
def test_switches_leave_the_words_alone(monkeypatch, p, n, name):
    """README: "same words" under every launch-shape switch.  n = 16 runs plain products and stand-alone inner products."""
    monkeypatch.setenv("BLZ_HEAVY_THR", "64")
    if name != "reorder_plain":
        monkeypatch.setenv("BLZ_NO_REORDER", "1")
    for key, val in SWITCHES[name].items():
        monkeypatch.setenv(key, val)
    if name.startswith("mfma"):
        # the shape of the matrix-core update is read once per process and device: a fresh process
        code = f"import test_gpu_fused_dot as t; t.switch_case({p}, {n}, {name!r}); print('child ok')"
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(q for q in sys.path if q))
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "child ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    else:
        switch_case(p, n, name)
