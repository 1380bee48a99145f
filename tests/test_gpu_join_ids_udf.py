"""-m gpu, through the host-side UDF mirror (libfreddy_host.so): knn_in_ivpq_batch by query ids (knn_in_ivpq_batch_ids) and the batch
form of analogy_3cosadd_in_ivpq.  The first is compared with knn_join over the gathered vectors and with the oracle, the second with
the loop of single analogy_3cosadd_in_ivpq calls, triple by triple."""
import numpy as np
import pytest

from test_gpu_udf import N, db, same  # noqa: F401  (db: that module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", [0, 1, 2])
def test_knn_in_ivpq_batch_ids(db, oracle, method):
    """argument order, an unknown id yields nothing, a duplicate is answered again, rows carry the query's id"""
    s, t = db
    asked = np.array([900, 17, 17, 15000, N + 5000, 3, -4, 12345], np.int32)
    known = np.array([900, 17, 17, 15000, 3, 12345], np.int32)
    targets = np.random.default_rng(3).choice(np.arange(1, N + 1), 3000, replace=False).astype(np.int32)
    s.set_alpha(3); s.set_pvf(4); s.set_method_flag(method)
    try:
        rows = s.knn_in_ivpq_batch_ids(asked, 5, targets)
        qs = t["x"][known - 1]
        exp, _ = oracle.ivpq_search_in(t["ivpq"], qs, 5, targets, 3, 4, method)
        assert rows["query_id"].tolist() == np.repeat(known, 5).tolist()
        same(rows, exp)
        by_vectors = s.knn_join(qs, known, 5, targets)
        assert np.array_equal(rows["query_id"], by_vectors["query_id"]) and np.array_equal(rows["id"], by_vectors["id"])
        assert np.array_equal(rows["distance"].view(np.uint32), by_vectors["distance"].view(np.uint32))
        assert len(s.knn_in_ivpq_batch_ids(np.array([N + 1, -1], np.int32), 5, targets)) == 0          # only unknown ids: no rows
        assert len(s.knn_in_ivpq_batch_ids(np.empty(0, np.int32), 5, targets)) == 0
    finally:
        s.set_alpha(10); s.set_pvf(20); s.set_method_flag(0)


def test_analogy_3cosadd_in_ivpq_batch(db):
    s, t = db
    rng = np.random.default_rng(8)
    input_ids = np.sort(rng.choice(np.arange(1, N + 1), 400, replace=False)).astype(np.int32)
    triples = rng.choice(np.arange(1, N + 1), (40, 3)).astype(np.int32)
    triples[:6] = [(10, 200, 3000), (4321, 4322, 77), (5, 5, 5), (int(input_ids[0]), int(input_ids[1]), int(input_ids[2])), (N + 7, 1, 2), (3, -1, 9)]
    s.set_pvf(6); s.set_alpha(3); s.set_method_flag(0)
    try:
        for ids in (input_ids, input_ids[:3], np.empty(0, np.int32)):
            loop = np.array([s.analogy_3cosadd_in_ivpq(int(a), int(b), int(c), ids) for a, b, c in triples], np.int32)
            got = s.analogy_3cosadd_in_ivpq_batch(triples, ids)
            assert np.array_equal(got, loop), (ids.size, got.tolist(), loop.tolist())
            assert (got[4:6] == -1).all()                                           # an unknown input id: the SQL's NULL
        assert (loop == -1).all()                                                   # no targets, no answer
        assert s.analogy_3cosadd_in_ivpq_batch(np.empty((0, 3), np.int32), input_ids).size == 0
    finally:
        s.set_pvf(20); s.set_alpha(10)
