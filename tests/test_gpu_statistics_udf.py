"""-m gpu: create_statistics / freddy_set_statistics_table of the host mirror (include/freddy_udf.h) through freddy_amd.udf:
the row a session computes equals the numpy model (tests/statistics_model.py) bit for bit and is installed; a session whose
stat table was rewritten answers ivpq_search_in as a session loaded with that table, without pinning again; and a stat table
freddy_load_ivpq refuses is refused here with the same words."""
import ctypes as C

import numpy as np
import pytest

import statistics_inputs as si
import statistics_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def udf():
    from freddy_amd import udf as u
    u.load()
    return u


def _session(udf, stats):
    t = si.tables()
    s = udf.Session()
    s.load_vecs_norm(t["ids"], t["vectors"])
    s.load_ivpq(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], stats)
    return s


def _device_row(s):
    """the row the pinned handle holds on the device"""
    ix = s.gpu_index("ivpq")
    out = np.empty(si.cells() + 1, np.float32)
    assert ix.lib.freddy_gpu_get_statistics(ix.h, out.ctypes.data_as(C.c_void_p), out.size) == 0
    return out


def _same_row(got, exp, what):
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), what


def _search(s, method=0):
    k, alpha = si.CALLS[0]
    qid = np.arange(1, si.Q + 1, dtype=np.int32)
    return s.ivpq_search_in(si.queries(), qid, k, si.targets(), alpha, si.PVF, method, True, si.CONFIDENCE, 10000000)


def test_create_statistics_equals_the_model_and_is_installed(udf):
    t = si.tables()
    s = _session(udf, si.row_b())
    handle = s.gpu_index("ivpq").h.value
    _same_row(_device_row(s), si.row_b(), "the row the session was loaded with")
    got = s.create_statistics()
    _same_row(got, sm.create_statistics(t["ids"], t["coarse_id"], si.cells())[0], "every row once")
    _same_row(_device_row(s), si.row_a(), "installed: the whole-table row")
    got = s.create_statistics(si.column())
    _same_row(got, si.row_b(), "the column's row, with multiplicity and unknown ids")
    _same_row(_device_row(s), si.row_b(), "installed: the column's row")
    with pytest.raises(udf.FreddyError, match="total is 0"):
        s.create_statistics(np.array([si.N + 7, -1], np.int32))
    with pytest.raises(udf.FreddyError, match="total is 0"):
        s.create_statistics(np.zeros(0, np.int32))
    _same_row(_device_row(s), si.row_b(), "a refused call leaves the row in force")
    assert s.gpu_index("ivpq").h.value == handle, "the handle was pinned again"
    s.close()


def test_set_statistics_table_answers_as_a_session_loaded_with_that_table(udf):
    a, b = _session(udf, si.row_a()), _session(udf, si.row_b())
    handle = a.gpu_index("ivpq").h.value
    before = _search(a)
    assert before.tobytes() != _search(b).tobytes(), "the two rows give the same answer: the case does not bite"
    a.set_statistics_table(si.row_b())
    _same_row(_device_row(a), si.row_b(), "the device's row")
    for method in si.METHODS:
        assert _search(a, method).tobytes() == _search(b, method).tobytes(), method
    assert a.gpu_index("ivpq").h.value == handle, "the handle was pinned again"
    a.close(); b.close()


def test_a_stat_table_load_ivpq_refuses_is_refused_alike(udf):
    t = si.tables()
    cells = si.cells()
    s = _session(udf, si.row_a())
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    pos, code, vec, n, sub = udf._entries(t["codebook"])
    cpos, ccode, cvec, cn, _ = udf._entries(t["coarse"])
    ids, cid, codes = (np.ascontiguousarray(t[k]) for k in ("ids", "coarse_id", "codes"))

    def both(sid, freq, words):
        sid, freq = np.ascontiguousarray(sid, np.int32), np.ascontiguousarray(freq, np.float32)
        assert s.lib.freddy_set_statistics_table(s.h, p(sid), p(freq), sid.size) == -1
        msg = s.lib.freddy_udf_last_error().decode()
        other = udf.Session()
        assert other.lib.freddy_load_ivpq(other.h, p(pos), p(code), p(vec), n, sub, p(cpos), p(ccode), p(cvec), cn, p(ids), p(cid), p(codes),
                                          C.c_int64(ids.size), p(sid), p(freq), sid.size) == -1
        assert msg == other.lib.freddy_udf_last_error().decode() and words in msg, msg
        other.close()
        _same_row(_device_row(s), si.row_a(), "a refused table leaves the row in force")

    row = si.row_b()
    both(np.arange(cells), row[:cells], f"has {cells} rows, expected {cells + 1}")
    both(np.arange(cells + 2), np.concatenate([row, [0.0]]), f"has {cells + 2} rows, expected {cells + 1}")
    sid = np.arange(cells + 1); sid[3] = cells + 1
    both(sid, row, "coarse_id out of range")
    sid = np.arange(cells + 1); sid[0] = -1
    both(sid, row, "coarse_id out of range")
    assert s.lib.freddy_set_statistics_table(s.h, None, p(row), row.size) == -1
    # rows in any order are one table: position = coarse_id
    order = np.random.default_rng(0).permutation(cells + 1)
    assert s.lib.freddy_set_statistics_table(s.h, p(np.ascontiguousarray(order, np.int32)), p(np.ascontiguousarray(row[order])), row.size) == 0
    _same_row(_device_row(s), row, "a shuffled stat table")
    s.close()
    empty = udf.Session()
    with pytest.raises(udf.FreddyError, match="not loaded"):
        empty.set_statistics_table(row)
    with pytest.raises(udf.FreddyError, match="not loaded"):
        empty.create_statistics()
    empty.close()
