"""CPU check of tests/redo_inputs.py: the conditions under which tests/test_gpu_redo_paths.py is neither vacuous (a hot input
that does not overflow a candidate buffer tests nothing) nor flaky (a healthy input near the copies could overflow too, and the
tests assert WHICH passes and queries are redone).  analogy_model and the oracle alone; nothing here needs a device.

Why GAP = 0.05 is a condition and not a measurement: the filter's candidates are the rows whose approximate score reaches the
threshold minus a bracket of EXF_EPS X |q| <= 6e-5 X |q| (exact2.h:25-31), about 1e-4 on this normalised table.  A healthy
input whose k-th best score lies 0.05 above the copies' score keeps every copy out of its candidates with a margin of hundreds
of brackets; another seed or table is valid exactly when this file still passes.

Exact kNN and the join take their threshold from the k-th best of the 1024 LANES' best sample rows (exf_threshold_kernel:
sample row i belongs to lane i mod 1024), which lies below the k-th best row when two of the k best share a lane.
candidates_bound() restates that rule in float64 and counts the rows within GAP of it: an upper bound of a healthy query's
candidates that has to stay under half the buffer."""
import numpy as np
import pytest

import analogy_model as am
import redo_inputs as ri

METHODS = ["3cosadd", "3cosmul"]


def test_table_and_call_layout():
    x, ids = ri.table()
    assert x.shape == (ri.N, ri.D) and (np.diff(ids) > 0).all() and (ids % 2 == 1).all()
    assert ri.COPY_ROWS.size == 10001 > ri.CAP and (x[ri.COPY_ROWS] == x[ri.ORIGINAL]).all()
    others = np.setdiff1d(np.arange(ri.N), ri.COPY_ROWS)
    assert not (x[others] == x[ri.ORIGINAL]).all(1).any(), "a row outside COPY_ROWS holds the copied vector"
    assert all(u not in set(ids.tolist()) for u in ri.UNKNOWN_IDS)
    # the live numbering, in which the passes of 32 are cut, differs from the caller's from the first unknown id on: the hot
    # triple at live position 63 (pass 1) sits at caller position 65 -- pass 2, were the redo cut in the caller's numbering
    call = ri.analogy_call({32: ri.HOT_TRIPLES[0], 41: ri.HOT_TRIPLES[1], 63: ri.HOT_TRIPLES[2]})
    assert call["triples"].shape == (73, 3) and call["live"].size == ri.N_LIVE
    assert call["live"][[0, 2, 32, 41, 63, 69]].tolist() == [0, 3, 33, 43, 65, 72]
    known = np.isin(call["triples"], ids).all(1)
    assert np.nonzero(~known)[0].tolist() == list(ri.UNKNOWN_AT)
    assert np.array_equal(call["triples"][call["live"]], ids[call["rows"]])
    assert (ri.healthy_triples() < ri.ORIGINAL).all(1).sum() == ri.N_LIVE - 1 and tuple(ri.healthy_triples()[3]) == ri.NEAR_MISS
    for kind, ok in (("nan", np.isnan), ("inf", np.isinf), ("big", lambda v: np.isfinite(v) & (np.abs(v) > 3e38))):
        q = ri.bad_query(x[5], kind)
        assert ok(q).sum() == 1 and np.array_equal(np.delete(q, 17), np.delete(x[5], 17)), kind


@pytest.mark.parametrize("method", METHODS)
def test_hot_triples_have_only_copies_on_top(method):
    """All of the model's 32 best rows are copies, in ascending id order, with ONE score: the copies that are not inputs tie for
    the best score, and there are more of them than a candidate buffer holds."""
    _, ids = ri.table()
    lists = ri.analogy_lists(method)
    for t in ri.HOT_TRIPLES:
        li, ls = lists[t]
        assert np.isin(li, ids[ri.COPY_ROWS]).all() and (np.diff(li) > 0).all(), (method, t)
        assert np.unique(ls.view(np.uint64)).size == 1, (method, t)
        assert li.tolist() == ri.lowest_copy_ids(t, ri.K_MAX).tolist(), (method, t)
        assert not np.isin(li, ids[list(t)]).any()
        assert np.setdiff1d(ri.COPY_ROWS, np.array(t)).size == 10000 > ri.CAP
    assert lists[ri.HOT_TRIPLES[1]][0][0] == ids[ri.ORIGINAL], "w3 a copy: row 4999 stays a candidate and has the lowest id"
    assert lists[ri.HOT_TRIPLES[0]][0][0] == ids[5000], "w3 = row 4999: excluded"


@pytest.mark.parametrize("method", METHODS)
def test_healthy_triples_stay_clear_of_the_copies(method):
    """At k = 32 the k-th best score exceeds the score of the copy vector by GAP; the copy's score comes from the model run over
    ONE copy id (a table cut behind row 5000 holds every input row of a healthy triple and that copy: the same chains)."""
    x, ids = ri.table()
    lists = ri.analogy_lists(method)
    t = ri.healthy_triples()
    ci, cs = am.model(x[:5001], ids[:5001], ids[t], 1, method, subset_ids=[ids[5000]])
    assert (ci[:, 0] == ids[5000]).all()
    gaps = np.array([lists[tuple(r)][1][ri.K_MAX - 1] for r in t.tolist()]) - cs[:, 0]
    print(f"{method}: smallest gap at k = 32 over {len(t)} healthy triples: {gaps.min():.4f}")
    assert gaps.min() >= ri.GAP, (method, np.argmin(gaps), gaps.min())
    assert not any(np.isin(lists[tuple(r)][0], ids[ri.COPY_ROWS]).any() for r in t.tolist())


def test_assembled_lists_are_the_models():
    """analogy_expected() puts per-triple lists of one model call together; the model over the call's own 73 triples says the same."""
    x, ids = ri.table()
    call = ri.analogy_call({32: ri.HOT_TRIPLES[0], 41: ri.HOT_TRIPLES[1], 63: ri.HOT_TRIPLES[2]})
    ei, es = ri.analogy_expected(call, 5, "3cosadd")
    mi, ms = am.model(x, ids, call["triples"], 5, "3cosadd")
    assert np.array_equal(ei, mi) and np.array_equal(es.view(np.uint64), ms.view(np.uint64))
    assert (ei[list(ri.UNKNOWN_AT)] == -1).all() and np.isneginf(es[list(ri.UNKNOWN_AT)]).all()


# ---- queries: exact kNN over the table, the join over a target set ---------------------------------------------------------
def candidates_bound(s, k):
    """s: similarities of one query to the searched rows in table order (float64).  -> (tau, rows within GAP of tau): the
    threshold rule of exf_threshold_kernel over the sample (whole strips of 32 rows, at most 32 768; all of them here)."""
    n_sample = min(s.size // 32, 1024) * 32
    assert n_sample // 32 == s.size // 32, "the sample is strided: restate the stride here"
    lane_best = np.full(1024, -np.inf)
    np.maximum.at(lane_best, np.arange(n_sample) % 1024, s[:n_sample])
    tau = -np.sort(-lane_best)[k - 1]
    return tau, int((s >= tau - ri.GAP).sum())


def check_queries(oracle, rows, qs, hot, what):
    """rows: the searched table rows, ascending.  Healthy queries: the oracle's 32nd best similarity over `rows` exceeds the
    similarity of one copy by GAP, and at most half a buffer of rows comes within GAP of the threshold.  Hot queries: the copies
    hold the best similarity, the threshold equals it, and they outnumber the buffer."""
    x, ids = ri.table()
    x64 = x.astype(np.float64)
    copies = np.intersect1d(rows, ri.COPY_ROWS)
    gaps = []
    for qi, q in enumerate(qs):
        s = x64[rows] @ q.astype(np.float64)
        tau, n = candidates_bound(s, ri.K_MAX)
        if qi in hot:
            e = oracle.exact_knn(x, ids, q, ri.K_MAX, ids[rows])
            assert e["id"].tolist() == ids[copies[:ri.K_MAX]].tolist() and np.unique(e["dist"].view(np.uint32)).size == 1, (what, qi)
            assert copies.size > ri.CAP and tau == s[np.searchsorted(rows, ri.ORIGINAL)] == s.max(), (what, qi)
            continue
        kth = oracle.exact_knn(x, ids, q, ri.K_MAX, ids[rows])["dist"][ri.K_MAX - 1]
        if copies.size:
            gaps.append(kth - oracle.exact_knn(x, ids, q, 1, ids[copies[:1]])["dist"][0])
        assert n <= ri.CAP // 2, (what, qi, n)
    if gaps:
        print(f"{what}: smallest gap at k = 32 over {len(gaps)} healthy queries: {min(gaps):.4f}")
        assert min(gaps) >= ri.GAP, (what, int(np.argmin(gaps)), min(gaps))


def test_search_queries(oracle):
    check_queries(oracle, np.arange(ri.N), ri.queries(hot_at=(3,)), {3}, "exact kNN")
    assert np.array_equal(ri.queries(Q=1, hot_at=(0,))[0], ri.hot_query())


def test_join_queries_and_targets(oracle):
    _, ids = ri.table()
    t = ri.overflow_targets()
    rows = np.nonzero(np.isin(ids, t))[0]
    assert rows.tolist() == list(range(4000, 16000)) and t.size == 12002
    check_queries(oracle, rows, ri.join_queries(), set(ri.JOIN_HOT_AT), "join over the copies")
    assert (ri.join_query_rows() < ri.ORIGINAL).all() and np.unique(ri.join_query_rows()).size == ri.JOIN_Q
    h = ri.healthy_targets()
    rows = np.nonzero(np.isin(ids, h))[0]
    assert rows.size == 9000 and not np.isin(rows, ri.COPY_ROWS).any() and h.size == 9002
    check_queries(oracle, rows, ri.queries(), set(), "join over 9 000 rows that are no copies")
