"""tests/mutation_model.py against the definition it restates: after any sequence of ivf appends the lists are the
concatenation of all rows ordered by (cell, id) -- appended ids ascend beyond every pinned id, so "the end of its cell's list"
and "ascending id inside the list" are the same order."""
import numpy as np
import pytest

import mutation_model as mm


def _rows(rng, n, first_id, C, m, K, gap=3):
    ids = (first_id + np.cumsum(rng.integers(1, gap + 1, size=n))).astype(np.int32)
    return ids, rng.integers(0, C, size=n).astype(np.int32), rng.integers(0, K, size=(n, m)).astype(np.int16)


@pytest.mark.parametrize("C,m,K,n0", [(7, 5, 16, 40), (32, 12, 256, 500), (4, 1, 3, 1)])
def test_ivf_appends_equal_the_lexsort_of_the_concatenation(C, m, K, n0):
    rng = np.random.default_rng(C * 100 + m)
    coarse = rng.standard_normal((C, 2 * m)).astype(np.float32)
    cb = rng.standard_normal((m, K, 2)).astype(np.float32)
    ids, cell, codes = _rows(rng, n0, 0, C, m, K)
    cell[cell == C - 1] = 0                              # the last cell is empty at the start
    model = mm.IVFModel.from_rows(coarse, cb, ids, cell, codes)
    assert model.list_len(C - 1) == 0
    all_ids, all_cell, all_codes = [ids], [cell], [codes]
    for n in (1, 63, 64, 65, 300, 2 * model.N + 3):
        a_ids, a_cell, a_codes = _rows(rng, n, int(all_ids[-1][-1]), C, m, K)
        if n == 65:
            a_cell[:] = C - 1                            # the empty cell fills up
        model.append(a_ids, a_cell, a_codes)
        all_ids.append(a_ids); all_cell.append(a_cell); all_codes.append(a_codes)
        cat_ids, cat_cell, cat_codes = np.concatenate(all_ids), np.concatenate(all_cell), np.concatenate(all_codes)
        order = np.lexsort((cat_ids, cat_cell))
        lo, m_ids, m_codes = model.tables()
        assert lo.tolist() == np.concatenate([[0], np.cumsum(np.bincount(cat_cell, minlength=C))]).tolist()
        assert np.array_equal(m_ids, cat_ids[order]) and np.array_equal(m_codes, cat_codes[order])
        assert m_ids.dtype == np.int32 and m_codes.dtype == np.int16 and lo.dtype == np.int32
        for c in range(C):
            assert (np.diff(m_ids[lo[c]:lo[c + 1]].astype(np.int64)) > 0).all(), c
        assert model.N == cat_ids.size and model.max_id == int(cat_ids.max())


def test_flat_kinds_keep_id_order_and_refusals_change_nothing():
    rng = np.random.default_rng(3)
    m, K = 3, 8
    cb = rng.standard_normal((m, K, 2)).astype(np.float32)
    ids = np.array([2, 5, 9], np.int32)
    codes = rng.integers(0, K, size=(3, m)).astype(np.int16)
    pq = mm.PQModel(cb, ids, codes)
    pq.append([10, 20], codes[:2])
    assert pq.ids.tolist() == [2, 5, 9, 10, 20] and np.array_equal(pq.codes[3:], codes[:2])
    before = (pq.ids.copy(), pq.codes.copy(), pq.codebook.copy())
    bad_code = codes[:2].copy(); bad_code[1, 2] = K
    for call, row in ((lambda: pq.append([21, 21], codes[:2]), "row 1"), (lambda: pq.append([20], codes[:1]), "row 0"),
                      (lambda: pq.append([30, 31], bad_code), "row 1"), (lambda: pq.append([30], None), "required"),
                      (lambda: pq.update_codebook(None), "required")):
        with pytest.raises(mm.Refused, match=row):
            call()
        assert np.array_equal(pq.ids, before[0]) and np.array_equal(pq.codes, before[1]) and np.array_equal(pq.codebook, before[2])
    pq.update_codebook(cb + 1)
    assert np.array_equal(pq.codebook, cb + 1)
    coarse = rng.standard_normal((2, 4, 3)).astype(np.float32)
    iv = mm.IVPQModel(cb, coarse, np.arange(1, 4), [0, 15, 3], codes, rng.standard_normal((3, 6)), np.zeros(17))
    assert iv.ids_affine
    with pytest.raises(mm.Refused, match="row 1"):
        iv.append([4, 5], [0, 16], codes[:2], np.zeros((2, 6)))
    with pytest.raises(mm.Refused, match="required"):
        iv.append([4], [0], codes[:1])
    assert iv.N == 3
    iv.append([4], [1], codes[:1], np.ones((1, 6)))
    assert iv.ids_affine
    iv.append([7], [1], codes[:1], np.ones((1, 6)))
    assert not iv.ids_affine and iv.vectors.shape == (5, 6) and iv.cell.tolist() == [0, 15, 3, 1, 1]
    v = mm.VecModel([1, 2], np.zeros((2, 4)))
    with pytest.raises(mm.Refused):
        v.update_codebook(cb)
    with pytest.raises(mm.Refused, match="required"):
        v.append([3])
    v.append([3, 8], np.ones((2, 4)))
    assert v.ids.tolist() == [1, 2, 3, 8] and v.vectors[2:].min() == 1.0
