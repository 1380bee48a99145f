"""-m gpu: the redo half of exact kNN's filter + refine on its two newer routes -- lists of 33 .. 1024 rows (option
exact_filter_k: exf_rank_threshold_kernel, exf_refine_tree_kernel<V> with its own copy of the last-workgroup epilogue) and wide
rows (option exact_wide: exf_wide_filter_kernel).  tests/test_gpu_redo_paths.py's shape: a query whose candidate buffer overflows,
or that is not finite, sits at a chosen place among healthy queries; the all-exact kernels answer that call, and LATER calls on
the same handle -- which read the verdict words, the arrival counter and the overflow flag the call's last workgroup must leave
at zero -- are filtered again.  Every list, ids and similarity bits, is the oracle's.

Which calls are redone is asserted from what tests/test_wide_redo_inputs_cpu.py proves about tests/wide_redo_inputs.py (the hot
query has more tied candidates than a buffer holds for every k; a healthy one keeps the copies 0.05 below its k-th best), and
read from the handle's profile."""
import functools

import numpy as np
import pytest

import wide_redo_inputs as wi
from test_gpu_redo_paths import _profiled, _same_lists       # (_same_lists compares NaN similarities as one pattern: _nan_as_one)

pytestmark = pytest.mark.gpu
SCAN = {"exact_scan", "exact_merge"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _filter_kernels(wide, k):
    return {"exact_filter_wide" if wide else "exact_filter", "exact_refine", "exact_threshold_rank" if k > 32 else "exact_threshold"}


def _k_max(wide):
    return wi.WIDE_K_MAX if wide else wi.NARROW_K_MAX


@functools.lru_cache(maxsize=None)
def _knn(oracle, wide):
    """expected lists of the table's largest k, computed once: the healthy queries' and the hot query's (a shorter list is a prefix)"""
    x, ids = wi.table(wide)
    K = _k_max(wide)
    return dict(healthy=[oracle.exact_knn(x, ids, q, K) for q in wi.queries(wide)], hot=oracle.exact_knn(x, ids, wi.hot_query(wide), K))


def _expected(oracle, wide, qs, at, bad):
    x, ids = wi.table(wide)
    knn = _knn(oracle, wide)
    exp = list(knn["healthy"][:len(qs)])
    for i in at:
        exp[i] = knn["hot"] if bad is None else oracle.exact_knn(x, ids, qs[i], _k_max(wide))
    return exp


def _pin(gpu, wide):
    x, ids = wi.table(wide)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_wide", int(wide))
    idx.set_option("exact_filter_k", 1024)
    return idx


def _call(idx, oracle, wide, qs, k, at, bad, what):
    """one search: redone (at not empty: the filter ran, then the all-exact kernels answered) or filtered; the oracle's lists"""
    (gi, gs), prof = _profiled(idx, lambda: idx.search(qs, k))
    names = set(prof)
    assert _filter_kernels(wide, k) <= names, (what, sorted(names))
    assert (SCAN <= names) if at else not (SCAN & names), (what, sorted(names))
    _same_lists(gi, gs, _expected(oracle, wide, qs, at, bad), k, what)


@pytest.mark.parametrize("Q,at", wi.HOT_AT)
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_one_hot_or_bad_query_then_a_healthy_call(gpu, oracle, wide, Q, at):
    """The query at `at` (pass tile 0, tile 1, the last of the pass of 64, the first and the last of the pass of 6, a call of
    one) overflows its buffer or is not finite; then a healthy call on the same handle, which must be the filter's."""
    idx = _pin(gpu, wide)
    for bad in (None,) + wi.POISONS:
        qs = wi.queries(wide, Q, hot_at=(at,), bad=bad)
        for k in (wi.WIDE_KS if wide else wi.NARROW_KS):
            what = f"wide={wide} Q={Q} at={at} bad={bad} k={k}"
            _call(idx, oracle, wide, qs, k, (at,), bad, what)
            _call(idx, oracle, wide, wi.queries(wide, Q), k, (), None, what + ": the healthy call behind it")
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_calls_after_a_fallback_alternating_the_refine_kernels(gpu, oracle, wide):
    """fallback, healthy, fallback, healthy, with k = 5 and k = 100 in turn: exf_refine_kernel<1> and exf_refine_tree_kernel<2>
    inherit each other's verdict words, arrival counter and overflow flag.  A stale word sends a healthy call to the all-exact
    kernels (seen in the profile) or lets a call trust lists it must not (seen in the lists)."""
    idx = _pin(gpu, wide)
    steps = [(100, (3,), None, 70), (5, (), None, 70), (5, (40,), "nan", 70), (100, (), None, 70),
             (5, (66,), None, 70), (100, (), None, 70), (100, (69,), "pos_inf", 70), (5, (), None, 1),
             (100, (0,), "all_nan", 1), (100, (), None, 1), (5, (), None, 70)]
    for n, (k, at, bad, Q) in enumerate(steps):
        qs = wi.queries(wide, Q, hot_at=at, bad=bad)
        _call(idx, oracle, wide, qs, k, at, bad, f"wide={wide} step {n + 1}: k={k} Q={Q} at={at} bad={bad}")
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_refining_every_row_removes_the_overflow(gpu, oracle, wide):
    """check_brackets bit 2: a buffer of N rows, so the hot query is the filter's own work at k > 32 and on the wide route too"""
    idx = _pin(gpu, wide)
    idx.set_option("check_brackets", 4)
    qs = wi.queries(wide, hot_at=(40,))
    exp = _expected(oracle, wide, qs, (40,), None)
    for k in (wi.WIDE_KS if wide else wi.NARROW_KS):
        c0 = idx.bound_checked()
        (gi, gs), prof = _profiled(idx, lambda: idx.search(qs, k))
        assert _filter_kernels(wide, k) <= set(prof) and not (SCAN & set(prof)), (wide, k, sorted(prof))
        _same_lists(gi, gs, exp, k, f"wide={wide} every row refined k={k}")
        assert idx.bound_checked() - c0 == wi.N_LIVE * wi.N
    assert idx.bound_violations() == 0
    idx.close()
