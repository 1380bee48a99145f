"""CPU check of tests/wide_redo_inputs.py: the conditions under which tests/test_gpu_exact_redo_variants.py is neither vacuous
(a hot query that does not overflow its buffer tests nothing) nor flaky (a healthy query near the copies could overflow too, and the
tests assert which calls are redone).  The oracle and float64 alone.

The threshold of a list of k > 32 rows is the exact k-th largest approximate similarity of the sample (csrc/exact_rank.h), and the
sample of a 20 000-row table is the table (625 full strips, all sampled); candidates are the rows that reach it minus a bracket of
about 1e-4 on these normalised tables (tests/test_redo_inputs_cpu.py: why GAP = 0.05 is a condition, not a measurement).  For
k <= 32 the threshold is the k-th best of the 1024 lanes' bests: test_redo_inputs_cpu.candidates_bound restates that rule."""
import numpy as np
import pytest

import exact_variant_inputs as vi
import redo_inputs as ri
import test_redo_inputs_cpu as rc
import util
import wide_redo_inputs as wi


def test_the_buffer_holds_8192_rows_for_every_k():
    for k in range(1, 1025):
        assert vi.filter_plan_k(wi.N, k) == (wi.N, 1, wi.CAP), k         # the sample is the table, the buffer min(N, max(8192, 4 k))
    assert wi.COPY_ROWS.size == 10001 > wi.CAP


@pytest.mark.parametrize("wide", [False, True])
def test_table_layout(wide):
    x, ids = wi.table(wide)
    assert x.shape == (wi.N, wi.WIDE_D if wide else ri.D) and x.nbytes <= 42 * 10 ** 6
    assert (np.diff(ids) > 0).all() and (x[wi.COPY_ROWS] == x[wi.ORIGINAL]).all()
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert 0.999 < norms.min() and norms.max() < 1.001                   # normalised rows: the bracket is about 1e-4
    rows = wi.healthy_rows(wide)
    assert np.unique(rows).size == wi.N_LIVE and (rows < wi.ORIGINAL).all()
    if wide:
        assert (wi.WIDE_D + 15) // 16 == 33 and wi.WIDE_D > 512 and wi.WIDE_D % 4 == 0
    for kind in wi.POISONS:
        q = wi.bad_query(x[5], kind)
        bad = ~np.isfinite(q)
        assert bad.sum() == (q.size if kind == "all_nan" else 1) and np.array_equal(q[~bad], x[5][~bad]), kind
        assert (np.isnan(q[bad]) if "nan" in kind else np.isposinf(q[bad])).all(), kind
    assert set(wi.POISONS) <= set(util.QUERY_POISONS)


def test_redo_inputs_queries_needed_a_replacement():
    """tests/redo_inputs.py's own healthy queries keep their distance at k = 32 and 40, not at k = 100 and 600"""
    x, _ = ri.table()
    s = x.astype(np.float64) @ ri.queries().astype(np.float64).T
    gap = lambda k: (-np.partition(-s, k - 1, axis=0)[k - 1] - s[ri.ORIGINAL]).min()
    assert gap(40) >= ri.GAP and gap(100) < ri.GAP and gap(600) < ri.GAP


@pytest.mark.parametrize("wide", [False, True])
def test_healthy_queries_keep_their_distance(oracle, wide):
    x, ids = wi.table(wide)
    x64 = x.astype(np.float64)
    K = wi.WIDE_K_MAX if wide else wi.NARROW_K_MAX
    gaps = []
    for qi, q in enumerate(wi.queries(wide)):
        s = x64 @ q.astype(np.float64)
        tau = -np.partition(-s, K - 1)[K - 1]                            # the rank rule at the largest k: the lowest threshold
        assert int((s >= tau - wi.GAP).sum()) <= wi.CAP // 2, (wide, qi)
        assert rc.candidates_bound(s, ri.K_MAX)[1] <= wi.CAP // 2, (wide, qi)      # the lane rule of k <= 32
        kth = oracle.exact_knn(x, ids, q, K)["dist"][K - 1]
        gaps.append(kth - oracle.exact_knn(x, ids, q, 1, ids[wi.ORIGINAL:wi.ORIGINAL + 1])["dist"][0])
    print(f"wide={wide}: smallest gap at k = {K} over {len(gaps)} healthy queries: {min(gaps):.4f}")
    assert min(gaps) >= wi.GAP, (wide, int(np.argmin(gaps)), min(gaps))


@pytest.mark.parametrize("wide", [False, True])
def test_the_hot_query_overflows_for_certain(oracle, wide):
    x, ids = wi.table(wide)
    K = wi.WIDE_K_MAX if wide else wi.NARROW_K_MAX
    q = wi.hot_query(wide)
    e = oracle.exact_knn(x, ids, q, K)
    assert e["id"].tolist() == ids[wi.COPY_ROWS[:K]].tolist() and np.unique(e["dist"].view(np.uint32)).size == 1
    s = x.astype(np.float64) @ q.astype(np.float64)
    for k in (wi.WIDE_KS if wide else wi.NARROW_KS):
        tau = -np.partition(-s, k - 1)[k - 1]
        assert tau == s[wi.ORIGINAL] == s.max() and int((s >= tau).sum()) >= wi.COPY_ROWS.size > wi.CAP, (wide, k)
    tau, _ = rc.candidates_bound(s, ri.K_MAX)
    assert tau == s.max()
    for Q, at in wi.HOT_AT:
        assert np.array_equal(wi.queries(wide, Q, hot_at=(at,))[at], q) and at < Q
