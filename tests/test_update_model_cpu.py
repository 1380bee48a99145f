"""tests/update_model.py against the definition it restates, and freddy_gpu_update_rows' argument errors, without a GPU.

The models: after any sequence of update / remove / append the tables are those built from scratch out of the rows with the new
payloads in place (flat kinds: id order; ivf: ordered by (cell, id)), N and max_id as before the update, and the oracle
answers the same over both.  The library: a NULL handle (with n = 0 too, as remove_rows treats it), n < 0 and NULL ids with
n > 0 return FREDDY_E_ARG before any device is touched; the bindings and the host mirror export the new verb."""
import ctypes

import numpy as np
import pytest

import update_model as um
import util


def _same_answers(oracle, got, exp):
    assert np.array_equal(got["id"], exp["id"]) and np.array_equal(got["dist"].view(np.uint32), exp["dist"].view(np.uint32))


def test_ivf_model_equals_the_lists_of_the_replaced_rows_and_the_oracle_agrees(oracle):
    t, x = util.shape_ivf_tables(100, 5, 64, 16, 6000), util.shape_corpus(6000, 100).numpy()
    C = 16
    cell = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)
    ids, codes = t["ids"].copy(), t["codes"].copy()
    n0 = 4000
    alive = ids <= n0
    model = um.IVFModel.from_rows(t["coarse"], t["codebook"], ids[alive], cell[alive], codes[alive])
    rng = np.random.default_rng(3)
    qs = np.ascontiguousarray(x[rng.choice(6000, 12, replace=False)])
    changed_a_list = False
    for step in ("codes", "move", "top", "rm", "append", "mixed", "all"):
        before = oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3)
        max_id, n_rows = model.max_id, model.N
        if step == "rm":
            gone = ids[alive][::7]
            assert model.remove(gone) == gone.size
            alive &= ~np.isin(ids, gone)
        elif step == "append":
            late = np.nonzero(ids > model.max_id)[0]
            late = late[np.argsort(ids[late])][:500]
            model.append(ids[late], cell[late], codes[late])
            alive[late] = True
        else:
            rows = np.nonzero(alive)[0]
            pick = {"codes": rows[::9], "move": rows[1::11], "top": rows[ids[rows] == model.max_id], "mixed": rows[2::5], "all": rows}[step]
            pick = pick[rng.permutation(pick.size)]
            new_codes = codes[rng.choice(6000, pick.size)]
            new_cell = cell[pick].copy()
            if step in ("move", "top"):
                new_cell = (new_cell + 1 + rng.integers(0, C - 1, pick.size)).astype(np.int32) % C
            elif step == "mixed":
                new_cell[::2] = (new_cell[::2] + 3) % C
            elif step == "all":
                new_cell = rng.permutation(C).astype(np.int32)[new_cell]
            ask_ids = np.concatenate([ids[pick], [10 ** 8, int(ids.max()) + 9]]).astype(np.int64)
            ask_cell = np.concatenate([new_cell, [0, C - 1]]).astype(np.int32)
            ask_codes = np.concatenate([new_codes, codes[:2]])
            assert model.update(ask_ids, ask_cell, ask_codes) == pick.size and pick.size > 0
            cell[pick], codes[pick] = new_cell, new_codes
            assert model.max_id == max_id and model.N == n_rows
        scratch = um.IVFModel.from_rows(t["coarse"], t["codebook"], ids[alive], cell[alive], codes[alive])
        for a, b in zip(model.tables(), scratch.tables()):
            assert np.array_equal(a, b) and a.dtype == b.dtype, step
        assert np.array_equal(model.cell_of(ids[alive]), cell[alive])
        got = oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3)
        _same_answers(oracle, got, oracle.ivfadc_search_many(scratch.oracle_table(oracle), qs, 5, 3))
        changed_a_list |= not np.array_equal(got["id"], before["id"])
    assert changed_a_list
    for bad, words in ((([5, 9, 5], [0, 1, 2], codes[:3]), "id 5 is listed twice, at positions 0 and 2"),
                       (([5, -9], [0, 1], codes[:2]), "id -9 at position 1"),
                       (([5, 9], [0, C], codes[:2]), "coarse_id out of range at new row 1"),
                       (([5, 9], [0, 1], np.full((2, 5), 64, np.int16)), "code out of range at new row 0"),
                       (([5, 9], None, codes[:2]), "required"), (([5, 9], [0, 1], None), "required")):
        tables = [a.copy() for a in model.tables()]
        with pytest.raises(um.Refused, match=words):
            model.update(*bad)
        assert all(np.array_equal(a, b) for a, b in zip(tables, model.tables()))
    assert model.update([], [], np.zeros((0, 5), np.int16)) == 0


def test_flat_models_replace_the_payload_in_place_and_the_oracle_agrees(oracle):
    t, x = util.shape_pq_tables(35, 7, 16, 6000), util.shape_corpus(6000, 35).numpy()
    ids = (t["ids"] * 2).astype(np.int32)
    codes = t["codes"][:900].copy()
    pq = um.PQModel(t["codebook"], ids[:900], codes)
    rng = np.random.default_rng(4)
    pick = rng.choice(900, 60, replace=False)
    new = t["codes"][1000:1060]
    ask = np.concatenate([ids[pick], [1, 3, 10 ** 8]])
    assert pq.update(ask, np.concatenate([new, new[:3]])) == 60 and pq.N == 900
    codes[pick] = new
    assert np.array_equal(pq.ids, ids[:900]) and np.array_equal(pq.codes, codes)
    _same_answers(oracle, oracle.pq_search(pq.oracle_table(oracle), x[5], 6), oracle.pq_search(oracle.pq_table(t["codebook"], ids[:900], codes), x[5], 6))
    pq.append([int(pq.ids[-1]) + 1], new[:1])             # the largest id is the one from before the update
    assert pq.update([int(pq.ids[-1])], new[5:6]) == 1 and np.array_equal(pq.codes[-1], new[5])
    assert pq.remove(ids[pick[:5]]) == 5 and pq.update(ids[pick[:5]], new[:5]) == 0
    with pytest.raises(um.Refused, match="id 8 is listed twice, at positions 1 and 2"):
        pq.update([2, 8, 8], new[:3])
    with pytest.raises(um.Refused, match="code out of range at new row 1"):
        pq.update([2, 10 ** 8], np.array([new[0], np.full(7, 16)], np.int16))   # an unknown id's payload is validated too
    with pytest.raises(um.Refused, match="required"):
        pq.update([2])

    v = um.VecModel(ids[:200], x[:200])
    assert v.update([ids[199], ids[0], 7], x[300:303]) == 2 and v.N == 200
    exp = x[:200].copy(); exp[199], exp[0] = x[300], x[301]
    assert np.array_equal(v.vectors, exp) and v.ids.tolist() == ids[:200].tolist()
    _same_answers(oracle, oracle.exact_knn(*v.oracle_table(oracle), x[300], 5), oracle.exact_knn(exp, ids[:200], x[300], 5))
    nan_row = np.full((1, 35), np.nan, np.float32)
    assert v.update([ids[4]], nan_row) == 1 and np.isnan(v.vectors[4]).all()     # vectors are accepted whatever their values
    with pytest.raises(um.Refused, match="required"):
        v.update([ids[4]])

    jt = util.shape_ivpq_tables(64, 8, 16, 4, 8000)
    for vec in (jt["vectors"][:300], None):
        iv = um.IVPQModel(jt["codebook"], jt["coarse"], jt["ids"][:300], jt["coarse_id"][:300], jt["codes"][:300], vec, jt["stats"])
        src = np.array([400, 401, 402])
        ask = np.array([int(jt["ids"][299]), int(jt["ids"][0]), 10 ** 8])
        assert iv.update(ask, jt["coarse_id"][src], jt["codes"][src], None if vec is None else jt["vectors"][src]) == 2
        for name, had, table in (("cell", iv.cell, jt["coarse_id"]), ("codes", iv.codes, jt["codes"])) + (() if vec is None else (("vectors", iv.vectors, jt["vectors"]),)):
            exp = table[:300].copy(); exp[299], exp[0] = table[400], table[401]
            assert np.array_equal(had, exp), name
        assert iv.ids_affine and iv.N == 300 and np.array_equal(iv.ids, jt["ids"][:300])
        with pytest.raises(um.Refused, match="coarse_id out of range at new row 0"):
            iv.update([int(jt["ids"][3])], [iv.cells], jt["codes"][:1], None if vec is None else jt["vectors"][:1])
        if vec is not None:
            with pytest.raises(um.Refused, match="required"):
                iv.update([int(jt["ids"][3])], [0], jt["codes"][:1])


def test_update_rows_argument_errors_are_reported_without_a_gpu():
    from freddy_amd import gpu
    lib = gpu.load()
    ids = np.array([1, 2, 3], np.int32)
    codes = np.zeros((3, 12), np.int16)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_upd = ctypes.c_int64(77)
    assert lib.freddy_gpu_update_rows(None, 3, p(ids), None, p(codes), None, ctypes.byref(n_upd)) == -1
    assert b"NULL" in lib.freddy_gpu_last_error()
    assert n_upd.value == 77                              # a refused call writes nothing
    assert lib.freddy_gpu_update_rows(None, 0, None, None, None, None, None) == -1      # n = 0 does not excuse a NULL handle
    assert b"NULL" in lib.freddy_gpu_last_error()
    assert lib.freddy_gpu_update_rows(None, -1, p(ids), None, p(codes), None, None) == -1
    assert b"n = -1" in lib.freddy_gpu_last_error()
    assert lib.freddy_gpu_update_rows(None, 3, None, None, p(codes), None, None) == -1
    assert b"no ids" in lib.freddy_gpu_last_error()
    assert "freddy_gpu_update_rows" in gpu.EXPORTS and hasattr(gpu._Index, "update_rows")


def test_host_mirror_exports_update_rows():
    from freddy_amd import udf
    lib = udf.load()
    assert hasattr(lib, "update_rows") and hasattr(udf.Session, "update_rows")
    s = udf.Session()
    ids = np.array([4, 9, 4], np.int32)
    v = np.zeros((3, 8), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.update_rows(s.h, p(ids), p(v), ctypes.c_int64(3), 8, None) != 0
    assert b"id 4 is listed twice, at positions 0 and 2" in lib.freddy_udf_last_error()
    ids[2] = -6
    assert lib.update_rows(s.h, p(ids), p(v), ctypes.c_int64(3), 8, None) != 0
    assert b"id -6 at position 2" in lib.freddy_udf_last_error()
    assert lib.update_rows(s.h, None, p(v), ctypes.c_int64(1), 8, None) != 0 and lib.update_rows(None, None, None, ctypes.c_int64(0), 8, None) != 0
    assert s.update_rows([7, 9], v[:2]) == 0              # nothing is loaded: nothing changes
    s.close()
