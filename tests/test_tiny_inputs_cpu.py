"""-m "not gpu": the cases of tests/tiny_inputs.py are what they claim, and they can tell a bracket that is too narrow from a
sound one by the result lists alone (oracle and numpy only; nothing of the library runs here)."""
import numpy as np
import pytest

import tiny_inputs as ti


def test_shapes_and_ids():
    ids, x, qs = ti.base()
    assert x.shape == (ti.N, ti.D) and qs.shape == (ti.Q, ti.D) and ids.shape == (ti.N,)
    assert ti.N == 65 * 32 and ti.Q == 64 + 6
    assert np.all(np.diff(ids) > 1), "ids ascend with gaps"
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert 0.5 < norms.min() and norms.max() < 2.0, "unit-scale rows"
    # the scalings are exact until the elements leave the normal range
    for name, (te, qe, _, _) in ti.CASES.items():
        _, t, q = ti.case(name)
        assert np.array_equal(q.astype(np.float64), qs.astype(np.float64) * 2.0 ** qe), name
        if te == "mixed":
            assert np.array_equal(t[:1000], x[:1000]) and np.array_equal(t[1100:], x[1100:]), name
            assert np.array_equal(t[ti.MIXED_ROWS].astype(np.float64), x[ti.MIXED_ROWS].astype(np.float64) * 2.0 ** -80), name
        elif te > -126 + 24:
            assert np.array_equal(t.astype(np.float64), x.astype(np.float64) * 2.0 ** te), name
        else:
            assert np.all(np.abs(t[t != 0]) < 2.0 ** -126) and np.count_nonzero(t) > t.size // 2, (name, "subnormal elements")


@pytest.mark.parametrize("name", sorted(ti.CASES))
def test_sums_of_squares_are_what_the_case_claims(name):
    _, t, q = ti.case(name)
    longest = int(np.argmax(np.linalg.norm(t.astype(np.float64), axis=1)))
    assert ti.classify(ti.fma_chain_of_squares(t[longest])) == ti.CASES[name][2], name
    assert ti.classify(ti.fma_chain_of_squares(q[0])) == ti.CASES[name][3], name
    if name in ti.NORM_VANISHES:
        assert "zero" in ti.CASES[name][2:], name


@pytest.mark.parametrize("name", sorted(ti.CASES))
def test_cluster_is_a_near_tie_the_reference_orders(oracle, name):
    ids, t, q = ti.case(name)
    cluster_ids = ids[ti.CLUSTER]
    n = cluster_ids.size
    assert n == 200
    e = oracle.exact_knn(t, ids, q[0], n, cluster_ids)
    assert len(e) == n and np.isfinite(e["dist"]).all(), name
    distinct = np.unique(e["dist"].view(np.uint32)).size
    if name in ti.MASSIVE_TIES:
        assert distinct == 1 and 0 < e["dist"][0] < 2.0 ** -126 and np.array_equal(e["id"], cluster_ids), (name, distinct)
    else:
        assert distinct >= 20 and np.all(e["dist"] >= 2.0 ** -126), (name, distinct)
    # query 0's best rows of the whole table are cluster rows
    top = oracle.exact_knn(t, ids, q[0], 32)
    assert set(top["id"].tolist()) <= set(cluster_ids.tolist()), name
    # all 200 within the filter's proven relative width of the fifth
    t64, q64 = t.astype(np.float64), q[0].astype(np.float64)
    s64 = t64 @ q64
    fifth = np.sort(s64)[-5]
    width = 2.7e-5 * np.linalg.norm(t64[ti.CLUSTER], axis=1) * np.linalg.norm(q64)
    assert np.all(np.abs(s64[ti.CLUSTER] - fifth) <= width), name


@pytest.mark.parametrize("name", ti.NORM_VANISHES)
def test_a_bracket_of_1e37_drops_a_true_member(oracle, name):
    """The model of a filter whose bracket is only the floor: a = the exact dot product rounded to binary32, candidates = rows
    with a >= (5th largest a) - 2e-37, ordered by the reference's bits.  Its list differs from the reference's top 5."""
    ids, t, q = ti.case(name)
    a = (t.astype(np.float64) @ q[0].astype(np.float64)).astype(np.float32)
    tau = np.sort(a)[-5]
    keep = np.nonzero(a >= tau - np.float32(2e-37))[0]
    assert 5 <= keep.size < 200, (name, keep.size)
    got = oracle.exact_knn(t, ids, q[0], 5, ids[keep])
    exp = oracle.exact_knn(t, ids, q[0], 5)
    assert len(got) == 5 and len(exp) == 5
    assert not np.array_equal(got["id"], exp["id"]), name
    assert not set(exp["id"].tolist()) <= set(ids[keep].tolist()), (name, "a member of the true list was filtered out")
