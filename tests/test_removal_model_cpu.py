"""tests/removal_model.py against the definition it restates, and freddy_gpu_remove_rows' argument errors, without a GPU.

The models: after any sequence of remove / append the tables are those built from scratch out of the rows that are left
(flat kinds: id order; ivf: ordered by (cell, id)), and the oracle answers the same over both.  The library: a NULL handle,
n < 0 and NULL ids with n > 0 return FREDDY_E_ARG before any device is touched; the host mirror exports delete_rows."""
import ctypes

import numpy as np
import pytest

import removal_model as rm
import util


def _sequence(rng, ids):
    """removals that mix pinned ids, unknown ids and duplicates, in no order"""
    some = rng.choice(ids, size=max(1, ids.size // 5), replace=False)
    return np.concatenate([some, some[:3], [int(ids.max()) + 7, 10 ** 8]]).astype(np.int64)[rng.permutation(some.size + 5)]


def test_ivf_model_equals_the_lists_of_the_remaining_rows_and_the_oracle_agrees(oracle):
    t, x = util.shape_ivf_tables(100, 5, 64, 16, 6000), util.shape_corpus(6000, 100).numpy()
    C, m = 16, 5
    cell = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)
    ids, codes = t["ids"], t["codes"]
    n0 = 4000
    first = np.nonzero(ids <= n0)[0]
    model = rm.IVFModel.from_rows(t["coarse"], t["codebook"], ids[first], cell[first], codes[first])
    alive = np.zeros(ids.size, bool); alive[first] = True
    rng = np.random.default_rng(1)
    qs = np.ascontiguousarray(x[rng.choice(6000, 12, replace=False)])
    late = np.nonzero(ids > n0)[0]
    late = late[np.argsort(ids[late])]
    for step in ("rm", "rm", "top", "append", "rm", "cell"):
        if step == "append":   # above the largest id that is LEFT: the model accepts it after the top went
            take = late[ids[late] > model.max_id][:700]
            model.append(ids[take], cell[take], codes[take])
            alive[take] = True
            continue
        if step == "top":
            want = np.array([model.max_id], np.int64)
        elif step == "cell":   # a whole cell
            want = model.list_ids[3].astype(np.int64)
        else:
            want = _sequence(rng, ids[alive])
        expect = int(np.isin(ids[alive], want).sum())
        assert model.remove(want) == expect and expect > 0
        alive &= ~np.isin(ids, want)
        scratch = rm.IVFModel.from_rows(t["coarse"], t["codebook"], ids[alive], cell[alive], codes[alive])
        for a, b in zip(model.tables(), scratch.tables()):
            assert np.array_equal(a, b) and a.dtype == b.dtype
        assert model.max_id == int(ids[alive].max()) and model.N == int(alive.sum())
        got = oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3)
        exp = oracle.ivfadc_search_many(scratch.oracle_table(oracle), qs, 5, 3)
        assert np.array_equal(got["id"], exp["id"]) and np.array_equal(got["dist"].view(np.uint32), exp["dist"].view(np.uint32))
        assert not np.isin(got["id"], want).any()
    assert model.list_len(3) == 0
    assert model.remove(np.concatenate(model.list_ids)) == int(alive.sum()) and model.N == 0 and model.max_id == -1


def test_flat_models_keep_id_order_and_the_oracle_agrees(oracle):
    t, x = util.shape_pq_tables(35, 7, 16, 6000), util.shape_corpus(6000, 35).numpy()
    ids = (t["ids"] * 2).astype(np.int32)
    pq = rm.PQModel(t["codebook"], ids[:900], t["codes"][:900])
    rng = np.random.default_rng(2)
    want = _sequence(rng, ids[:900])
    keep = ~np.isin(ids[:900], want)
    assert pq.remove(want) == int((~keep).sum())
    assert np.array_equal(pq.ids, ids[:900][keep]) and np.array_equal(pq.codes, t["codes"][:900][keep])
    q = x[5]
    got = oracle.pq_search(pq.oracle_table(oracle), q, 6)
    exp = oracle.pq_search(oracle.pq_table(t["codebook"], ids[:900][keep], t["codes"][:900][keep]), q, 6)
    assert np.array_equal(got["id"], exp["id"]) and np.array_equal(got["dist"].view(np.uint32), exp["dist"].view(np.uint32))
    pq.append([int(pq.ids[-1]) + 1], t["codes"][:1])     # right above the largest id that is left
    assert pq.remove([1, 3, 10 ** 8]) == 0 and pq.N == int(keep.sum()) + 1
    with pytest.raises(rm.Refused, match="id -1 at position 2"):
        pq.remove([2, 4, -1])
    assert pq.N == int(keep.sum()) + 1

    v = rm.VecModel(ids[:200], x[:200])
    assert v.remove([ids[0], ids[199], ids[0]]) == 2 and v.ids.tolist() == ids[1:199].tolist() and np.array_equal(v.vectors, x[1:199])
    got = oracle.exact_knn(*v.oracle_table(oracle), x[7], 5)
    exp = oracle.exact_knn(x[1:199], ids[1:199], x[7], 5)
    assert np.array_equal(got["id"], exp["id"]) and np.array_equal(got["dist"].view(np.uint32), exp["dist"].view(np.uint32))
    assert v.remove(v.ids) == 198 and v.N == 0
    v.append([5], x[:1])
    assert v.ids.tolist() == [5]

    jt = util.shape_ivpq_tables(64, 8, 16, 4, 8000)
    for vec in (jt["vectors"][:300], None):
        iv = rm.IVPQModel(jt["codebook"], jt["coarse"], jt["ids"][:300], jt["coarse_id"][:300], jt["codes"][:300], vec, jt["stats"])
        assert iv.ids_affine
        assert iv.remove(jt["ids"][295:300]) == 5 and iv.ids_affine          # the tail: still consecutive
        assert iv.remove(jt["ids"][:2]) == 2 and iv.ids_affine               # the head likewise
        assert iv.remove([int(jt["ids"][100]), 10 ** 8]) == 1 and not iv.ids_affine   # a hole
        keep = np.r_[2:100, 101:295]
        assert np.array_equal(iv.ids, jt["ids"][keep]) and np.array_equal(iv.cell, jt["coarse_id"][keep]) and np.array_equal(iv.codes, jt["codes"][keep])
        assert (iv.vectors is None) == (vec is None) and (vec is None or np.array_equal(iv.vectors, vec[keep]))
        with pytest.raises(rm.Refused):
            iv.remove([-5])
        assert iv.N == keep.size


def test_remove_rows_argument_errors_are_reported_without_a_gpu():
    from freddy_amd import gpu
    lib = gpu.load()
    ids = np.array([1, 2, 3], np.int32)
    gone = ctypes.c_int64(77)
    assert lib.freddy_gpu_remove_rows(None, 3, ids.ctypes.data_as(ctypes.c_void_p), ctypes.byref(gone)) == -1
    assert b"NULL" in lib.freddy_gpu_last_error()
    assert gone.value == 77                               # a refused call writes nothing
    assert lib.freddy_gpu_remove_rows(None, -1, ids.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert b"n = -1" in lib.freddy_gpu_last_error()
    assert lib.freddy_gpu_remove_rows(None, 3, None, None) == -1
    assert b"no ids" in lib.freddy_gpu_last_error()
    assert "freddy_gpu_remove_rows" in gpu.EXPORTS and hasattr(gpu._Index, "remove_rows")


def test_host_mirror_exports_delete_rows():
    from freddy_amd import udf
    lib = udf.load()
    assert hasattr(lib, "delete_rows") and hasattr(udf.Session, "delete_rows")
    s = udf.Session()
    ids = np.array([4, -2], np.int32)
    assert lib.delete_rows(s.h, ids.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(2), None) != 0
    assert b"id -2 at position 1" in lib.freddy_udf_last_error()
    assert lib.delete_rows(s.h, None, ctypes.c_int64(1), None) != 0 and lib.delete_rows(None, None, ctypes.c_int64(0), None) != 0
    assert s.delete_rows([7, 7, 9]) == 0                  # nothing is loaded: nothing leaves
    s.close()
