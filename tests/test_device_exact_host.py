"""The part of tests/test_gpu_device_exact.py that needs no GPU: device_exact.py restates on integers what the launchers of
csrc/blz_devalg.hip and blz_devsmall.hip decide, and the GPU file takes its shapes from it.  Held here:

  - reduce_model IS the reducer where csrc/modp.h says it is exact, and the all-(p-1) inputs of the GPU file are where one
    product too many (57 bits) or two too many (58 ... 62 bits) is a wrong word -- so the GPU cases ask for chunk + 2;
  - dot_rows_past_chunk gives every accumulator of k_dev_dot (one product or two) chunk + 2 products at 8, 256 and 304 compute units,
    and no smaller row count of that shape does;
  - the case lists reach every instantiation the launchers can produce (the table of DESIGN.md, "Device block algebra at
    the bounds").
"""
import random

import pytest

import device_exact as DX
import exact_ref as X

BARRETT = [p for p in DX.DEV_PRIMES if DX.barrett(p)]
TIGHT = (DX.P58, DX.P59, DX.P60, DX.P61B, DX.P62)  # the largest primes of 58 ... 62 bits
CLASSES = {"AccS": DX.P32, "fold61": DX.P61, "Barrett": DX.P57}


def test_the_primes_are_what_the_issue_names():
    assert sorted(DX.DEV_PRIMES) == sorted(set(DX.DEV_PRIMES)) and len(DX.DEV_PRIMES) == 15
    assert BARRETT == [DX.P32B, DX.P48, DX.P56, DX.P57, DX.P58, DX.P59, DX.P60, DX.P61B, DX.P62]
    assert [X.chunk(p) for p in BARRETT] == [64, 64, 64, 64, 31, 15, 7, 3, 1] and X.chunk(DX.P61) == 32
    assert all(X.is_prime(p) for p in DX.DEV_PRIMES)
    assert [p.bit_length() for p in DX.NEW_PRIMES] == [32, 33, 48, 56, 57, 58, 59, 60]
    assert {DX.acc_class(p) for p in DX.DEV_PRIMES} == set(CLASSES)
    assert all(DX.acc_class(p) == c for c, p in CLASSES.items())


@pytest.mark.parametrize("p", BARRETT, ids=DX.pid)
def test_the_model_is_the_reducer(p):
    """residue + j products of (p-1)^2, 0 <= j <= chunk: what an accumulator of the kernels holds when it is reduced"""
    rnd = random.Random(p)
    sq = (p - 1) ** 2
    for res in (0, 1, p - 1, rnd.randrange(p)):
        for j in range(X.chunk(p) + 1):
            T = res + j * sq
            assert T < 1 << (63 + p.bit_length())
            assert DX.reduce_model(T, p) == T % p, (res, j)
    bound = 1 << (63 + p.bit_length())
    for T in [bound - 1, bound - p, bound // 2] + [rnd.randrange(bound) for _ in range(2000)]:
        assert DX.reduce_model(T, p) == T % p, T
    for count in (0, 1, X.chunk(p), X.chunk(p) + 1, X.chunk(p) + 2, 3 * X.chunk(p) + 5):        # the chunk loop as the kernels have it
        assert DX.sum_model(count, p, X.chunk(p)) == count * sq % p
        assert DX.sum_model(count, p, X.chunk(p), start=p - 1) == (p - 1 + count * sq) % p


def test_the_inputs_are_sensitive():
    """all words p - 1: at 2^57 - 13 a sum of chunk + 1 products is a wrong word, at the largest primes of 58 ... 62 bits a
    sum of chunk + 1 is still right and one of chunk + 2 is wrong -- with or without a residue under the products"""
    p = DX.P57
    sq, c = (p - 1) ** 2, X.chunk(p)
    assert X.slack(p) == c == 64
    for res in (0, p - 1):
        T = res + (c + 1) * sq
        assert DX.reduce_model(T, p) != T % p
    for p in TIGHT:
        sq, c = (p - 1) ** 2, X.chunk(p)
        assert X.slack(p) == c + 1
        for res in (0, p - 1):
            assert DX.reduce_model(res + (c + 1) * sq, p) == (res + (c + 1) * sq) % p
            assert DX.reduce_model(res + (c + 2) * sq, p) != (res + (c + 2) * sq) % p
    # the loop with an off-by-one in it (a reduction every chunk + 1 products) on chunk + 2 products, the fewest any
    # accumulator of a "past the chunk" case takes: wrong at 57 bits, unseen at 58 ... 62; off by two is wrong everywhere
    for count in (X.chunk(DX.P57) + 2, 2 * X.chunk(DX.P57) + 7):
        assert DX.sum_model(count, DX.P57, X.chunk(DX.P57) + 1) != count * (DX.P57 - 1) ** 2 % DX.P57
    for p in TIGHT:
        count, sq = X.chunk(p) + 2, (p - 1) ** 2
        assert DX.sum_model(count, p, X.chunk(p) + 1) == count * sq % p
        assert DX.sum_model(count, p, X.chunk(p) + 2) != count * sq % p
    # the folding prime sees no overrun short of 2^128: its cases are there for the values
    assert X.slack(DX.P61) == 2 * X.chunk(DX.P61)


def test_the_figures_of_the_tiling():
    assert DX.dot_shape(8, 256) == (128, 1024, 16, 1, 2)
    assert DX.dot_shape(1, 256) == (1024, 1024, 256, 1, 1)
    assert DX.dot_shape(16, 256) == (64, 1024, 4, 1, 2)
    assert DX.dot_shape(17, 256) == (32, 1024, 1, 4, 1) and DX.dot_shape(32, 304)[1:] == (1024, 1, 4, 1)
    assert DX.dot_shape(33, 256) == (16, 962, 1, 16, 1) and DX.dot_shape(64, 256) == (16, 256, 1, 16, 1)
    assert DX.dot_rows_past_chunk(DX.P57, 8, 256) == 1179649
    assert DX.dot_rows_past_chunk(DX.P57, 64, 256) == 20481
    # what today's largest blocks give an accumulator at 256 compute units: the chunk branch fires at chunk <= 3 and 32 only
    assert DX.dot_products_per_accumulator(200003, 8, 256) == 8
    assert DX.dot_products_per_accumulator(1000, 8, 256) == 6        # eight workgroups of one tile, the last of 104 rows
    assert DX.dot_products_per_accumulator(4097, 64, 256) == 16      # (the 4097 rows of test_gpu_device_fused.py)


@pytest.mark.parametrize("cus", DX.PAST_CUS)
def test_the_row_counts_do_what_they_claim(cus):
    big = [p for p in BARRETT if p.bit_length() >= 57]
    assert set(big) | {DX.P61} == set(DX.PAST_PRIMES)
    for p in DX.PAST_PRIMES:
        want = X.chunk(p) + 2
        for n in DX.PAST_WIDTHS:
            TR, max_blocks, slices, _, _ = DX.dot_shape(n, cus)
            rows, T = DX.dot_rows_past_chunk(p, n, cus), DX.dot_tiles_past_chunk(p, n, cus)
            assert rows == T * max_blocks * TR + 1
            assert DX.dot_products_per_accumulator(rows, n, cus) >= want, (p, n)
            if T >= 2:                                  # the smallest of its shape: a tile fewer per workgroup falls short
                assert DX.dot_products_per_accumulator((T - 1) * max_blocks * TR + 1, n, cus) < want, (p, n)
            # the three blocks of a dot_pair case, at stride n; the 8-byte lane stride is n + 1, on one of two blocks
            assert 3 * rows * n * 8 < 512 << 20, (p, n, cus)
            assert rows * (2 * n + 1) * 8 < 512 << 20, (p, n, cus)


def test_the_combine_cases_pass_the_chunk():
    seen = {}
    for p, n, terms in DX.COMBINE_PAST:
        assert p in DX.PAST_PRIMES and terms * n >= X.chunk(p) + 2, (p, n, terms)
        masks = DX.past_masks(terms)
        assert len(masks) == terms and all(m[0] for m in masks) and sum(m[1] for m in masks) == max(terms - 1, 1)
        seen.setdefault(p, []).append((n, terms))
    assert set(seen) == set(DX.PAST_PRIMES)
    for need in ((DX.P57, [(32, 3), (48, 2), (64, 2), (64, 4)]), (DX.P58, [(12, 3), (16, 3)]), (DX.P59, [(8, 3)]), (DX.P60, [(5, 2)])):
        assert all(c in seen[need[0]] for c in need[1]), need
    # n = 5 and n = 6: runs of odd and even length, a run of ONE product, and a reduction in the middle of a term's row
    runs = [r for p, n, terms in DX.COMBINE_PAST if n in (5, 6) for r in DX.combine2_runs(X.chunk(p), n, terms)]
    assert {5, 6} <= {n for _, n, _ in DX.COMBINE_PAST}
    assert any(L == 1 for L, _ in runs) and any(L % 2 == 1 and L > 1 for L, _ in runs) and any(L % 2 == 0 for L, _ in runs)
    for p, n, terms in DX.COMBINE_PAST:
        got = DX.combine2_runs(X.chunk(p), n, terms)
        assert sum(L for L, _ in got) == n * terms and any(red for _, red in got), (p, n, terms)
        assert all(L <= X.chunk(p) for L, _ in got)
    # the 256 -> 1024 thread switch of both combine launchers at n = 48
    assert DX.combine_form(DX.P57, 48, 2, True).threads == 256 and DX.combine_form(DX.P57, 48, 3, True).threads == 1024
    assert DX.combine2_form(DX.P57, 48, ((1, 0), (0, 1)), True).threads == 256
    assert DX.combine2_form(DX.P57, 48, ((1, 0), (1, 1)), True).threads == 1024


def test_the_small_cases_pass_the_chunk_where_a_width_can():
    for p, n in DX.RREF_PAST:
        assert DX.barrett(p) and n - 1 >= X.chunk(p) + 2, (p, n)
    for need in ((DX.P58, 48), (DX.P58, 64), (DX.P59, 24), (DX.P59, 32), (DX.P60, 12), (DX.P60, 16), (DX.P61B, 8), (DX.P62, 4),
                 (DX.P62, 24)):
        assert need in DX.RREF_PAST
    assert X.chunk(DX.P57) + 2 > 64 - 1                 # 57 bits: no width passes the chunk in k_dev_rref
    # k_dev_chain's W * S with W = -(J + I) and S all p - 1: n - 1 products of (p-1)^2 and one of (p-2)(p-1) from zero
    for p, n in DX.CHAIN_PAST:
        c = X.chunk(p)
        assert n >= c + 2
        T = (c + 1) * (p - 1) ** 2 + (p - 2) * (p - 1)
        assert DX.reduce_model(T, p) != T % p and DX.reduce_model(T - (p - 1) ** 2, p) == (T - (p - 1) ** 2) % p, (p, n)
    assert (DX.P57, 24) in DX.RREF_VALUES and (DX.P57, 64) in DX.RREF_VALUES
    assert all(n - 1 < X.chunk(p) + 2 for p, n in DX.RREF_VALUES)


# ------------------------------------------------------------------------------------------------ every form is reached


def cells(acc, threads_lg):
    return {(acc, t, lg) for t, lgs in threads_lg.items() for lg in lgs}


def test_every_form_of_the_dots_is_reached():
    widths, lanes = range(1, 65), (True, False)
    can = {DX.dot_form(p, n, v) for p in CLASSES.values() for n in widths for v in lanes}
    table = {(acc, shape, ln) for acc in CLASSES for shape in ("TT=1", "TT=2", "NP=4", "NP=16") for ln in (8, 16)}
    assert can == {c for c in table if c[1:] != ("TT=1", 16)}      # n = 1 is odd: 8-byte lanes only
    can2 = {DX.dot2_form(p, n, v) for p in CLASSES.values() for n in widths for v in lanes}
    assert can2 == {c if c[:2] != ("Barrett", "NP=16") else ("Barrett", "two dot launches", c[2]) for c in can}
    got, got2 = set(), set()
    for p, n in DX.RANDOM_CASES + DX.DOT_EXTRA:
        for pads in DX.DOT_PADS:
            got.add(DX.dot_form(p, n, DX.pair_ok(n, pads[0]) and DX.pair_ok(n, pads[2])))
            got2.add(DX.dot2_form(p, n, all(DX.pair_ok(n, pd) for pd in pads)))
    assert got == can and got2 == can2, (can - got, can2 - got2)
    past, past2 = set(), set()                          # and past the chunk: every shape of the Barrett class, both lanes
    for p, n in DX.DOT_PAST:
        for v in lanes:
            past.add(DX.dot_form(p, n, v))
            past2.add(DX.dot2_form(p, n, v))
    assert {c for c in can if c[0] != "AccS"} == past and {c for c in can2 if c[0] != "AccS"} == past2


def test_every_form_of_the_combines_is_reached():
    widths, lanes = range(1, 65), (True, False)
    can = {DX.combine_form(p, n, k, v) for p in CLASSES.values() for n in widths for k in (1, 2, 3, 4) for v in lanes}
    assert can == set().union(*(cells(acc, {256: range(7), 1024: (5, 6)}) for acc in CLASSES))
    got = {DX.combine_form(p, n, k, DX.lanes16(n, pads, k))
           for p, n in DX.RANDOM_CASES + DX.COMBINE_EXTRA for k, pads in DX.combine_plan(n)}
    assert got == can, can - got
    # the fused kernel: the same cells (the 96-bit class keeps the 16-byte lanes at 1024 threads: lane groups of 16 too),
    # a term that reads its panels from global memory, and the 1024-thread launch that drops the 16-byte lanes
    forms = {(p, n, m, v): DX.combine2_form(p, n, m, v) for p in CLASSES.values() for n in widths for m in DX.ALL_MASKS for v in lanes}
    can2 = {f[:3] for f in forms.values()}
    want2 = set().union(*(cells(acc, {256: range(7), 1024: (4, 5, 6) if acc == "AccS" else (5, 6)}) for acc in CLASSES))
    assert can2 == want2
    assert {f.acc for f in forms.values() if not all(f.in_lds)} == set(CLASSES)
    assert {f.acc for f in forms.values() if f.dropped_vec2} == {"fold61", "Barrett"}
    mine = [DX.combine2_form(p, n, m, DX.lanes16(n, pads, len(m)))
            for p, n in DX.RANDOM_CASES + DX.COMBINE_EXTRA for m, pads in DX.pair_plan(n)]
    assert {f[:3] for f in mine} == can2, can2 - {f[:3] for f in mine}
    assert {f.acc for f in mine if not all(f.in_lds)} == set(CLASSES)
    assert {f.acc for f in mine if f.dropped_vec2} == {"fold61", "Barrett"}
    assert {(f.threads, f.lg) for f in mine if f.dropped_vec2 and f.acc == "Barrett"} == {(1024, 5), (1024, 6)}
    # past the chunk: both launch sizes, with and without the 16-byte lanes, a reduction inside the two-word loop's term
    past = {DX.combine_form(p, n, k, v) for p, n, k in DX.COMBINE_PAST for v in lanes}
    past2 = {DX.combine2_form(p, n, DX.past_masks(k), v) for p, n, k in DX.COMBINE_PAST for v in lanes}
    assert {("Barrett", t) for t in (256, 1024)} <= {f[:2] for f in past} and {("Barrett", t) for t in (256, 1024)} <= {f[:2] for f in past2}
    assert any(f.dropped_vec2 for f in past2)


def test_every_form_of_the_small_algebra_is_reached():
    assert {DX.chain_threads(n) for n in range(1, 65)} == {(64, 0), (64, 1), (64, 2), (64, 3), (256, 4), (1024, 5), (1024, 6)}
    got = {DX.chain_threads(n) for _, n in DX.SMALL_CASES}
    assert {(64, 1), (64, 2), (64, 3), (256, 4), (1024, 5), (1024, 6)} <= got      # 64, 256, 1024 at lg = 5 and at lg = 6
    for p in DX.FULL:
        assert {DX.chain_threads(n)[0] for q, n in DX.SMALL_CASES if q == p} == {64, 256, 1024}
        assert {DX.chain_threads(n) for q, n in DX.SMALL_CASES if q == p} >= {(1024, 5), (1024, 6)}
    assert {DX.rref_group(n) for n in range(1, 65)} == {1, 2, 4, 8, 16, 32, 64}
    assert {DX.rref_group(n) for _, n in DX.RREF_CASES} == {1, 2, 4, 8, 16, 32, 64}
    assert {DX.rref_group(n) for _, n in DX.RREF_RANDOM} == {1, 2, 4, 8, 16, 32, 64}
    assert all(rows[1] > n and rows[2] > 2 * DX.rref_tile_rows(n) for n in DX.FULL_WIDTHS for rows in [DX.rref_random_rows(n)])
    assert DX.rref_tile_rows(64) == 32 and DX.rref_tile_rows(4) == 512
    # the echelon block: 2 * (2 * CUs) * TR + 5 rows where a tile holds the n - 1 echelon rows, a third tile at n = 48 and 64
    assert [DX.rref_tiles(n) for n in (1, 2, 4, 8, 12, 16, 24, 32, 33, 48, 64)] == [2] * 9 + [3, 3]
    for _, n in DX.RREF_CASES:
        TR = DX.rref_tile_rows(n)
        assert (DX.rref_tiles(n) - 1) * TR >= n - 1 > (DX.rref_tiles(n) - 2) * TR - (n == 1)
        assert DX.rref_rows(n, 256) == DX.rref_tiles(n) * 512 * TR + 5


def test_the_iteration_cases():
    assert DX.ITER_CASES == [(24, (1 << 57) - 13), (32, (1 << 58) - 27), (12, (1 << 60) - 93), (2, (1 << 32) + 15), (4, (1 << 32) - 5)]
