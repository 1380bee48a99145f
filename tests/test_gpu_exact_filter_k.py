"""Option exact_filter_k: exact kNN as filter + refine for lists of 33 .. 1024 rows (csrc/exact_rank.h: the threshold by rank
selection, the refine stage's tree merge; exact_host.h filter_plan_k).  Every list is compared bit for bit with the oracle's."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
E_LIMIT = "freddy_gpu error -5"   # include/freddy_gpu.h FREDDY_E_LIMIT as gpu._check words it
BIG = 131072 + 77   # 4098 full strips: a sample of 65 536 rows (k = 33 .. 64) is every second strip


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _table(d, N):
    """test_gpu_exact_wide._table: duplicate rows, 70 queries, a negated one and one with copies in the table."""
    x = util.shape_corpus(N, d).numpy().astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::N // 70][:70].copy()
    qs[3] = -qs[3]
    qs[6] = x[100]
    return x, ids, qs


def _search(idx, qs, k):
    """(ids, similarities, names of the kernels launched)"""
    idx.profile_enable(True)
    gi, gs = idx.search(qs, k)
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return gi, gs, names


def _index(gpu, ids, x, **options):
    idx = gpu.VectorIndex(ids, x)
    for name, value in {"exact_wide": int(x.shape[1] > 512), "exact_filter_k": 1024, **options}.items():
        idx.set_option(name, value)
    return idx


def _filtered(names, d=32):
    return {"exact_threshold_rank", "exact_refine", "exact_filter_wide" if d > 512 else "exact_filter"} <= names and "exact_scan" not in names


@pytest.mark.parametrize("d", [32, 300, 516])
def test_lists_and_path(gpu, oracle, d):
    """both sides of every rung of pick_V; Q = 70: two passes, the second of 6 queries; d = 516: T = 33 through the wide filter"""
    x, ids, qs = _table(d, 8192 + 40)
    exp = [oracle.exact_knn(x, ids, q, 1024) for q in qs]
    idx = _index(gpu, ids, x)
    for Q in (1, 70):
        for k in (33, 64, 65, 128, 129, 512, 513, 1024):
            gi, gs, names = _search(idx, qs[:Q], k)
            util.assert_exact_lists(gi, gs, exp, k, f"d={d} Q={Q} k={k}")
            assert _filtered(names, d), (d, Q, k, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.fixture(scope="module")
def big():
    x, ids, qs = _table(32, BIG)
    return x, ids, qs[:9]


@pytest.mark.parametrize("k", [33, 64])
def test_strided_sample(gpu, oracle, big, k):
    x, ids, qs = big
    exp = [oracle.exact_knn(x, ids, q, k) for q in qs]
    idx = _index(gpu, ids, x)
    for cus in (0, 3):
        idx.set_option("grid_cus", cus)
        gi, gs, names = _search(idx, qs, k)
        util.assert_exact_lists(gi, gs, exp, k, f"k={k} grid_cus={cus}")
        assert _filtered(names), (k, cus, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("k", [34, 130])
def test_ties_at_the_kth_place(gpu, oracle, k):
    """every row four times under four ids (tests/join_bigk_inputs.py): places k - 1 .. k + 2 hold one similarity, id order decides"""
    N, period = 8400, 2100
    x = np.ascontiguousarray(util.shape_corpus(period, 300).numpy()[np.arange(N) % period])
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[5:period:300] + np.float32(0.01)
    exp = [oracle.exact_knn(x, ids, q, k + 1) for q in qs]
    assert all(e["dist"][k - 1] == e["dist"][k] for e in exp)
    idx = _index(gpu, ids, x)
    gi, gs, names = _search(idx, qs, k)
    util.assert_exact_lists(gi, gs, exp, k, f"ties k={k}")
    assert _filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()


@pytest.mark.parametrize("d", [32, 300])
def test_every_rows_bracket(gpu, oracle, d):
    x, ids, qs = _table(d, 8192 + 40)
    idx = _index(gpu, ids, x, check_brackets=4)
    gi, gs, names = _search(idx, qs[:12], 100)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, q, 100) for q in qs[:12]], 100, f"every row d={d}")
    assert _filtered(names) and idx.bound_violations() == 0, sorted(names)
    assert idx.bound_checked() == 12 * x.shape[0]
    idx.close()


def test_overflow_redo(gpu, oracle):
    """The sampled (even) strips hold rows nearly orthogonal to the query, the others perturbed copies of it: the sample's k-th
    best says nothing about them, more rows than the buffer holds pass, and the all-exact scan answers the call."""
    k, d, rng = 40, 32, np.random.default_rng(5)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    x = rng.standard_normal((BIG, d))
    x -= np.outer(x @ q, q) * 0.999
    sampled = ((np.arange(BIG) // 32) % 2 == 0) & (np.arange(BIG) < 4096 * 32)    # strips 0, 2, .., 4094
    x[~sampled] = q + 0.01 * rng.standard_normal((int((~sampled).sum()), d))
    x, qs = x.astype(np.float32), np.stack([q, -q]).astype(np.float32)
    ids = np.arange(1, BIG + 1, dtype=np.int32)
    s = x.astype(np.float64) @ qs[0].astype(np.float64)
    eps = 4e-5 * 1.001 * np.linalg.norm(x.astype(np.float64), axis=1).max() * np.linalg.norm(qs[0].astype(np.float64))
    assert int((s > np.sort(s[sampled])[-k] + eps).sum()) > 8192       # filter_plan_k: cap = max(8192, 4 * 40 * 3)
    idx = _index(gpu, ids, x)
    gi, gs, names = _search(idx, qs, k)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, v, k) for v in qs], k, "overflow")
    assert "exact_scan" in names, sorted(names)
    healthy = x[:128:64] + np.float32(0.01)                             # near two orthogonal rows: the copies score ~ 0
    gi, gs, names = _search(idx, healthy, k)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, v, k) for v in healthy], k, "after the overflow")
    assert _filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()


def test_option_and_defaults(gpu, oracle):
    N0, N1 = 8192 + 8, 8192 + 8 + 45
    x, ids, qs = _table(300, N1)
    x[N0 + 5] *= np.float32(300.0)                  # the append brings a larger element: the copy is laid out again
    qs = np.concatenate([qs[:9], x[N0 + 5:N0 + 6]])
    idx = gpu.VectorIndex(ids[:N0], x[:N0])
    for bad in (31, 1025):
        with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + rf".*exact_filter_k: {bad} "):
            idx.set_option("exact_filter_k", bad)
    assert "exact_scan" in _search(idx, qs, 33)[2]                      # the default: 32
    idx.set_option("exact_filter_k", 1024)
    names = _search(idx, qs, 32)[2]
    assert "exact_threshold" in names and "exact_threshold_rank" not in names and "exact_scan" not in names, sorted(names)
    exp0 = [oracle.exact_knn(x[:N0], ids[:N0], x[r], 100) for r in (7, 4000)]
    idx.profile_enable(True)
    qi, gi, gs = idx.exact_search_ids(ids[[7, 4000]], 100)
    assert _filtered(set(idx.profile_read())) and qi.tolist() == ids[[7, 4000]].tolist()
    idx.profile_enable(False)
    util.assert_exact_lists(gi, gs, exp0, 100, "by row id")
    idx.append_rows(ids[N0:], vectors=x[N0:])
    gi, gs, names = _search(idx, qs, 100)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, q, 100) for q in qs], 100, "after the append")
    assert _filtered(names) and idx.bound_violations() == 0, sorted(names)
    idx.close()
