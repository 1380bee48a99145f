"""-m "not gpu": what tests/test_gpu_exact_variants.py says about its shapes, derived from the host plans restated in
tests/exact_variant_inputs.py (csrc/exact_host.h filter_plan_k, csrc/exact_wide.h): strips, segments, rounds, sample rows."""
import exact_variant_inputs as vi

MI355X_CUS = 256


def test_wide_strips_and_segments():
    strips = (vi.WIDE_N + 31) // 32
    assert strips == 259 and strips % 2 == 1 and vi.WIDE_N - 258 * 32 == 13       # an odd count; the last strip holds 13 rows
    assert [(d + 15) // 16 for d in vi.WIDE_DS] == [33, 48, 128]
    assert vi.segments(516, 8) == [8, 8, 8, 8, 1] and vi.segments(516, 16) == [16, 16, 1]   # a short last segment for both
    assert vi.segments(768, 16) == [16, 16, 16] and vi.segments(768, 8) == [8] * 6          # full segments only
    assert len(vi.segments(2048, 8)) == 16 and len(vi.segments(2048, 16)) == 8              # the longest stream
    for TS, _, _ in vi.WIDE_SHAPES.values():
        assert TS % vi.EXF_PF == 0


def test_wide_walk_on_a_whole_device_and_on_three_cus():
    # R = 2: 17 workgroups of 16 strips, one round; the last workgroup has 3 strips: wave 0 two, wave 1 ONE live strip, six idle waves
    assert vi.wide_walk(vi.WIDE_N, 2, MI355X_CUS) == (17, 1, [2, 1, 0, 0, 0, 0, 0, 0], 0)
    # TS = 16: 33 workgroups of 8 strips; the last has 3 live waves
    assert vi.wide_walk(vi.WIDE_N, 1, MI355X_CUS) == (33, 1, [1, 1, 1, 0, 0, 0, 0, 0], 0)
    # grid_cus = 3, one workgroup per CU: 3 workgroups and several rounds.  240 strips fill ten rounds of 24 (five of 48); the 19
    # left are 8 + 8 + 3 under R = 1 -- idle waves, NO idle workgroup -- and 16 + 3 under R = 2: one idle workgroup
    assert vi.wide_walk(vi.WIDE_N, 1, 3) == (3, 11, [1, 1, 1, 0, 0, 0, 0, 0], 0)
    assert vi.wide_walk(vi.WIDE_N, 2, 3) == (3, 6, [2, 1, 0, 0, 0, 0, 0, 0], 1)
    # grid_cus = 4: 256 strips fill whole rounds, the 3 left are one workgroup's: three idle workgroups under either shape
    assert vi.wide_walk(vi.WIDE_N, 1, 4) == (4, 9, [1, 1, 1, 0, 0, 0, 0, 0], 3)
    assert vi.wide_walk(vi.WIDE_N, 2, 4) == (4, 5, [2, 1, 0, 0, 0, 0, 0, 0], 3)
    assert set(vi.WIDE_GRID_CUS) == {3, 4}
    # the default shape takes two workgroups per CU: six workgroups on three CUs (tests/test_gpu_exact_wide.py)
    assert vi.wide_walk(vi.WIDE_N, 0, 3)[0] == 6


def test_query_tiles():
    """Q -> (passes of 64, NT of the last pass): 1 and 9: one tile; 33: two tiles, the second with one query; 70: 64 + 6"""
    tiles = {Q: [(min(64, Q - q0), 1 if min(64, Q - q0) <= 32 else 2) for q0 in range(0, Q, 64)] for Q in vi.WIDE_QS}
    assert tiles == {1: [(1, 1)], 9: [(9, 1)], 33: [(33, 2)], 70: [(64, 2), (6, 1)]}


def test_small_table_sample_counts():
    plans = {(N, k): vi.filter_plan_k(N, k) for N, k, _ in vi.SMALL_TABLES}
    assert plans[(2080, 1024)] == (2080, 1, 2080)                 # the sample is the table; so is the buffer
    assert plans[(1000, 1024)].n_sample == 992 < 1024             # exf_rank_threshold_kernel: n_sample < k -> thr = -inf
    assert plans[(1000, 512)].n_sample == 992 > 512
    assert plans[(300, 512)] == (288, 1, 300)                     # fewer rows than k: n_sample < k too, lists padded from row 300 on
    assert plans[(31, 40)] == (0, 1, 31) and plans[(3, 64)] == (0, 1, 3)          # no full strip: n_sample = 0
    for (N, k), p in plans.items():
        assert p.cap == N, (N, k)                                 # every row fits the buffer: no overflow redo in these tables


def test_plan_of_the_larger_tables():
    """tests/test_gpu_exact_filter_k.py's figures: BIG rows at k = 33 .. 64 sample every second strip; 8232 rows: all full strips"""
    big = 131072 + 77
    assert vi.filter_plan_k(big, 33) == (65536, 2, 8192)
    assert vi.filter_plan_k(big, 40).cap == max(8192, 4 * 40 * 3)
    assert vi.filter_plan_k(8232, 1024) == (8224, 1, 8192)
    assert vi.filter_plan_k(8232, 5) == (8224, 1, 8192)
