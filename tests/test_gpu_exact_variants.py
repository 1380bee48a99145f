"""-m gpu: the kernels of exact kNN that only an option selects, and the forced small tables at k > 32.

a. exact_wide_shape = 1 and 2 (exf_wide_filter_kernel<NT, SAMPLE, 16, 1> and <NT, SAMPLE, 8, 2>, csrc/exact_wide.h) and
   exact_rank_hist = 1 (exf_rank_threshold_kernel<4>, csrc/exact_rank.h): documented options that no other test sets.
b. exact_filter = 1 with exact_filter_k = 1024 over tables smaller than the sample, than k and than a strip.
Every list is compared bit for bit with the oracle's exact_knn; every path claim is read from the handle's profile.  The shapes'
strips, segments, rounds and sample rows are derived in tests/test_exact_variant_inputs_cpu.py."""
import functools

import numpy as np
import pytest

import exact_variant_inputs as vi
import test_gpu_exact_filter_k as fk
import test_gpu_exact_wide as ew
import util

pytestmark = pytest.mark.gpu
U = np.uint32


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


_search = ew._search


def _wide_names(names, wide=True):
    return {"exact_filter_wide" if wide else "exact_filter", "exact_refine"} <= names and "exact_scan" not in names


@functools.lru_cache(maxsize=None)
def _wide_expected(oracle, d):
    """(table, ids, queries, the oracle's lists of 32) of one d, shared by both shapes"""
    x, ids, qs = ew._table(d, vi.WIDE_N)
    return x, ids, qs, [oracle.exact_knn(x, ids, q, 32) for q in qs]


# ---- a. the wide shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", vi.WIDE_DS)
@pytest.mark.parametrize("shape", [1, 2])
def test_wide_shape_lists_equal_the_oracle_and_shape_0(gpu, oracle, shape, d):
    """259 strips (odd: the last R = 2 wave has one live strip; the last strip holds 13 rows), T = 33 / 48 / 128, Q = 1, 9 (one
    tile), 33 (a second tile of one query), 70 (passes of 64 and 6), k = 1 and 32.  d = 768 again on grids of 3 and 4 workgroups:
    several rounds, the last with idle waves (3) and idle workgroups (4: under shape 1 the 19 strips of the last round of three
    workgroups are 8 + 8 + 3, no workgroup idles there -- tests/test_exact_variant_inputs_cpu.py)."""
    x, ids, qs, exp = _wide_expected(oracle, d)
    idx = ew._wide(gpu, ids, x)
    for cus in (0,) + (vi.WIDE_GRID_CUS if d == 768 else ()):
        idx.set_option("grid_cus", cus)
        for Q in vi.WIDE_QS:
            for k in (1, 32):
                what = f"shape={shape} d={d} Q={Q} k={k} grid_cus={cus}"
                idx.set_option("exact_wide_shape", shape)
                gi, gs, names = _search(idx, qs[:Q], k)
                util.assert_exact_lists(gi, gs, exp, k, what)
                assert _wide_names(names), (what, sorted(names))
                idx.set_option("exact_wide_shape", 0)
                hi, hs, names = _search(idx, qs[:Q], k)
                assert _wide_names(names), (what, sorted(names))
                assert np.array_equal(gi, hi) and np.array_equal(gs.view(U), hs.view(U)), (what, "differs from shape 0")
    idx.set_option("grid_cus", 0)
    # back and forth on one handle: every shape leaves the state the next one needs
    ref = None
    for s in (shape, 0, shape, 3 - shape, shape, 0):
        idx.set_option("exact_wide_shape", s)
        gi, gs, names = _search(idx, qs, 32)
        assert _wide_names(names), (s, sorted(names))
        if ref is None:
            ref = gi, gs
            util.assert_exact_lists(gi, gs, exp, 32, f"switching, shape {s}")
        assert np.array_equal(gi, ref[0]) and np.array_equal(gs.view(U), ref[1].view(U)), (shape, d, "after switching to", s)
    # every (query, row) pair refined and compared with its bracket
    Q = 12
    idx.set_option("exact_wide_shape", shape)
    idx.set_option("check_brackets", 4)
    v0, c0 = idx.bound_violations(), idx.bound_checked()
    gi, gs, names = _search(idx, qs[:Q], 5)
    util.assert_exact_lists(gi, gs, exp, 5, f"every row shape={shape} d={d}")
    assert _wide_names(names), sorted(names)
    assert idx.bound_violations() - v0 == 0 and idx.bound_violations() == 0
    assert idx.bound_checked() - c0 == Q * vi.WIDE_N
    idx.close()


def test_wide_shape_at_k_above_32(gpu, oracle):
    """the shapes meet the rank threshold and the tree refine too: d = 516, k = 100, Q = 70"""
    x, ids, qs, _ = _wide_expected(oracle, 516)
    exp = [oracle.exact_knn(x, ids, q, 100) for q in qs]
    idx = ew._wide(gpu, ids, x, exact_filter_k=1024)
    for shape in (1, 2):
        idx.set_option("exact_wide_shape", shape)
        gi, gs, names = _search(idx, qs, 100)
        util.assert_exact_lists(gi, gs, exp, 100, f"shape={shape} k=100")
        assert fk._filtered(names, 516), (shape, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


# ---- a. the histogram copies of the rank selection --------------------------------------------------------------------------
def test_rank_hist_lists(gpu, oracle):
    x, ids, qs = fk._table(32, 8192 + 40)
    exp = [oracle.exact_knn(x, ids, q, 1024) for q in qs]
    idx = fk._index(gpu, ids, x, exact_rank_hist=1)
    for Q in (1, 70):
        for k in (33, 64, 65, 512, 1024):
            gi, gs, names = _search(idx, qs[:Q], k)
            util.assert_exact_lists(gi, gs, exp, k, f"exact_rank_hist=1 Q={Q} k={k}")
            assert fk._filtered(names), (Q, k, sorted(names))
    # the option off again on the same handle: the same lists
    idx.set_option("exact_rank_hist", 0)
    gi, gs, names = _search(idx, qs, 65)
    util.assert_exact_lists(gi, gs, exp, 65, "exact_rank_hist back to 0")
    assert fk._filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()


def test_rank_hist_ties_at_the_kth_place(gpu, oracle):
    """tests/test_gpu_exact_filter_k.py test_ties_at_the_kth_place's table: places k - 1 .. k + 2 hold one similarity"""
    k, N, period = 34, 8400, 2100
    x = np.ascontiguousarray(util.shape_corpus(period, 300).numpy()[np.arange(N) % period])
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[5:period:300] + np.float32(0.01)
    exp = [oracle.exact_knn(x, ids, q, k + 1) for q in qs]
    assert all(e["dist"][k - 1] == e["dist"][k] for e in exp)
    idx = fk._index(gpu, ids, x, exact_rank_hist=1)
    gi, gs, names = _search(idx, qs, k)
    util.assert_exact_lists(gi, gs, exp, k, f"exact_rank_hist=1 ties k={k}")
    assert fk._filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()


def test_rank_hist_strided_sample(gpu, oracle):
    """BIG rows at k = 33: the sample is every second strip, 65 536 values per query through the four histograms"""
    x, ids, qs = fk._table(32, fk.BIG)
    qs = qs[:9]
    assert vi.filter_plan_k(fk.BIG, 33)[:2] == (65536, 2)
    idx = fk._index(gpu, ids, x, exact_rank_hist=1)
    gi, gs, names = _search(idx, qs, 33)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, q, 33) for q in qs], 33, "exact_rank_hist=1 strided sample")
    assert fk._filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()


# ---- b. forced small tables at k > 32 ----------------------------------------------------------------------------------------
def _small(N, d):
    x = np.ascontiguousarray(util.shape_corpus(2080, d).numpy()[:N])
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[[0, N // 2, N - 1]] + np.float32(0.01)
    return x, ids, qs


@pytest.mark.parametrize("N,k,what", vi.SMALL_TABLES + tuple((N, k, what + " (wide)") for N, k, what in vi.SMALL_WIDE))
def test_forced_small_tables_at_k_above_32(gpu, oracle, N, k, what):
    """exact_filter = 1 with exact_filter_k = 1024: the sample equals the table, has fewer rows than k (thr = -inf, every row a
    candidate), or none at all; a table with fewer rows than k pads its lists with (-1, -inf) behind the tree merge."""
    d = 516 if what.endswith("(wide)") else 300
    x, ids, qs = _small(N, d)
    exp = [oracle.exact_knn(x, ids, q, k) for q in qs]
    assert all(len(e) == min(N, k) for e in exp)
    idx = fk._index(gpu, ids, x, exact_filter=1)
    for Q in (1, 3):
        for brackets in (0, 4):
            idx.set_option("check_brackets", brackets)
            c0 = idx.bound_checked()
            gi, gs, names = _search(idx, qs[:Q], k)
            assert gi.shape == (Q, k)
            util.assert_exact_lists(gi, gs, exp, k, f"{what}: N={N} d={d} k={k} Q={Q} check_brackets={brackets}")
            assert fk._filtered(names, d), (what, Q, sorted(names))
            assert idx.bound_checked() - c0 == (Q * N if brackets else 0)
    assert idx.bound_violations() == 0
    idx.close()
