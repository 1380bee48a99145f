"""ctypes binding of the reference's own C code (oracle/_ref/libfreddy_ref.so), parallel to oracle/oracle.py.

TEST INFRASTRUCTURE ONLY.  The library is built by `make -C oracle ref` (build() runs it) from the reference's
source tree, our stand-in PostgreSQL headers (oracle/ref/pgshim/), the stand-in runtime (oracle/ref/pgshim_rt.c)
and our driver (oracle/ref/ref_driver.c).  It exists only where the reference tree is (or was) present and is
never committed; status() tells the tests which of the three situations they are in.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle.oracle import ENTRY, _f32, _i16, _i32, _p

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("FREDDY_REF_SO") or os.path.join(_HERE, "_ref", "libfreddy_ref.so")   # (tests/test_sanitizers.py: the ASan + UBSan build)
REFERENCE = os.environ.get("FREDDY_REFERENCE", "/root/reference")
STRLEN = 24


def tree_present():
    return os.path.exists(os.path.join(REFERENCE, "freddy_extension", "index_utils.c"))


def status():
    """'ok' (library there, or buildable), 'absent' (neither the tree nor a built library: the pins cannot run)."""
    if os.path.exists(_SO) or tree_present():
        return "ok"
    return "absent"


def build():
    if not os.environ.get("FREDDY_REF_SO") and tree_present():
        subprocess.check_call(["make", "-C", _HERE, "-s", "ref"])
    return _SO


class RefError(RuntimeError):
    """The reference raised an ERROR (elog), or the stand-in SPI refused a statement."""


class Ref:
    """Array-in/array-out access to the reference's functions and set-returning functions."""

    def __init__(self):
        self.lib = C.CDLL(build())      # a library that cannot be loaded raises: with the tree present that is a failure
        self.lib.fr_last_error.restype = C.c_char_p

    def _ck(self, rc):
        if rc != 0:
            raise RefError(self.lib.fr_last_error().decode(errors="replace"))

    # ---- function level --------------------------------------------------------------------------------
    def sqdist(self, a, b):
        a, b = _f32(a), _f32(b)
        out = C.c_float()
        self._ck(self.lib.fr_sqdist(_p(a), _p(b), a.size, C.byref(out)))
        return np.float32(out.value)

    def lut_entries(self, q, m, K, pos, code, vectors, double=False):
        pos, code, vectors, q = _i32(pos), _i32(code), _f32(vectors), _f32(q)
        s = vectors.shape[1]
        out = np.full((m // 2) * K * K if double else m * K, np.nan, np.float32)
        fn = self.lib.fr_lut_double if double else self.lib.fr_lut
        self._ck(fn(_p(out), m, K, s, _p(q), _p(pos), _p(code), _p(vectors)))
        return out

    def adc(self, lut, codes, K):
        lut, codes = _f32(lut), _i16(codes)
        out = C.c_float()
        self._ck(self.lib.fr_adc(_p(lut), _p(codes), codes.size, K, C.byref(out)))
        return np.float32(out.value)

    def topk_stream(self, dists, ids, k, sentinel, init_many=False):
        d, i = _f32(dists), _i32(ids)
        out = np.empty(k, ENTRY)
        self._ck(self.lib.fr_topk_stream(k, C.c_float(sentinel), d.size, _p(d), _p(i), int(init_many), _p(out)))
        return out

    def topkpv_stream(self, dists, ids, k, sentinel, init_many=False):
        """(entries, index of the stream element whose vector each slot carries)"""
        d, i = _f32(dists), _i32(ids)
        out, vi = np.empty(k, ENTRY), np.empty(k, np.int32)
        self._ck(self.lib.fr_topkpv_stream(k, C.c_float(sentinel), d.size, _p(d), _p(i), 4, int(init_many), _p(out), _p(vi)))
        return out, vi

    def sort_entries(self, entries, pv=False):
        e = np.ascontiguousarray(entries, ENTRY).copy()
        self._ck(self.lib.fr_sort_entries(_p(e), e.size, int(pv)))
        return e

    def cmp_entries(self, a, b, pv=False):
        out = C.c_int()
        self._ck(self.lib.fr_cmp_entries(C.c_float(float(a)), C.c_float(float(b)), int(pv), C.byref(out)))
        return out.value

    def postverify(self, q, k, pvf, cand_ids, cand_vecs, sentinel):
        q, ci, cv = _f32(q), _i32(cand_ids), _f32(cand_vecs)
        assert ci.size == k * pvf and cv.shape == (k * pvf, q.size)
        out = np.empty(k, ENTRY)
        self._ck(self.lib.fr_postverify(_p(q), q.size, k, pvf, _p(ci), _p(cv), C.c_float(sentinel), _p(out)))
        return out

    def multi_index_select(self, coarse, stats, queries, active, n_targets, min_target_count, confidence, multi=True):
        cq, st, qs, act = _f32(coarse), _f32(stats), _f32(queries), _i32(active)
        Kc = cq.shape[1] if multi else cq.shape[0]
        cells = Kc * Kc if multi else Kc
        assert st.size == cells + 1
        out = np.full((act.size, cells), -1, np.int32)
        cnt = np.zeros(act.size, np.int32)
        last = C.c_int()
        self._ck(self.lib.fr_multi_index_select(int(multi), _p(cq), Kc, qs.shape[1], _p(st), _p(qs), qs.shape[0], _p(act), act.size,
                                                n_targets, min_target_count, C.c_float(confidence), _p(out), _p(cnt),
                                                C.byref(last)))
        return [out[i, :cnt[i]].copy() for i in range(act.size)], bool(last.value)

    def confidence(self, expect, size, p, stat_size=0, hyp=True):
        out = C.c_float()
        self._ck(self.lib.fr_confidence(int(hyp), int(expect), int(size), C.c_float(float(p)), int(stat_size), C.byref(out)))
        return np.float32(out.value)

    def update_codebook(self, codebook, counts, vecs, order=None):
        """-> (in-memory codebook, counts, codes [n, m], count_incs [m*K]) after updateCodebook"""
        cb, cnt, v = _f32(codebook).copy(), _i32(counts).copy(), _f32(vecs)
        m, K, s = cb.shape
        od = _i32(np.arange(m * K) if order is None else order)
        codes = np.full((v.shape[0], m), -1, np.int32)
        incs = np.empty(m * K, np.int32)
        self._ck(self.lib.fr_update_codebook(_p(cb), _p(cnt), m, K, s, _p(v), v.shape[0], _p(od), _p(codes), _p(incs)))
        return cb, cnt, codes, incs

    def target_list(self, ids, list_size, method):
        ids = _i32(ids)
        out = np.empty(max(ids.size, 1), np.int32)
        sizes = np.empty(ids.size // list_size + 2, np.int32)
        n = C.c_int()
        self._ck(self.lib.fr_target_list(_p(ids), ids.size, list_size, method, _p(out), _p(sizes), C.byref(n)))
        return out[:ids.size], sizes[:n.value]

    def blacklist(self, add, ask):
        add, ask = _i32(add), _i32(ask)
        out = np.empty(max(ask.size, 1), np.int32)
        self._ck(self.lib.fr_blacklist(_p(add), add.size, _p(ask), ask.size, _p(out)))
        return out[:ask.size].astype(bool)

    def bytea_roundtrip(self, a, preallocated=False):
        a = np.ascontiguousarray(a)
        kind = {np.dtype(np.float32): 0, np.dtype(np.int32): 1, np.dtype(np.int16): 2}[a.dtype]
        out = np.zeros(max(a.size, 1), a.dtype)
        n, vs = C.c_int(), C.c_int()
        self._ck(self.lib.fr_bytea_roundtrip(kind, _p(a), a.size, int(preallocated), _p(out), C.byref(n), C.byref(vs)))
        return out[:n.value], vs.value

    def cosine_simple(self, a, b, norm=False):
        a, b = _f32(a), _f32(b)
        out = C.c_double()
        self._ck(self.lib.fr_cosine_simple(_p(a), _p(b), a.size, int(norm), C.byref(out)))
        return out.value

    def have_core_functions(self):
        return bool(self.lib.fr_have_core_functions())

    def _core(self, op, a, b):
        a = _f32(a)
        b = a if b is None else _f32(b)
        out = np.empty(max(a.size, 1), np.float32)
        self._ck(self.lib.fr_core_bytea(op, _p(a), _p(b), a.size, _p(out)))
        return out

    def cosine_similarity_bytea(self, a, b):
        return self._core(0, a, b)[0]

    def vec_minus(self, a, b):
        return self._core(1, a, b)[:np.size(a)]

    def vec_plus(self, a, b):
        return self._core(2, a, b)[:np.size(a)]

    def vec_normalize(self, a):
        return self._core(3, a, None)[:np.size(a)]

    # ---- tables ----------------------------------------------------------------------------------------
    def reset_tables(self):
        self.lib.fr_reset_tables()

    def set_w(self, W):
        self._ck(self.lib.fr_set_parameter(b"get_w()", int(W)))

    def add_codebook(self, table, codebook, entry_order=None):
        """codebook [m][K][s]; entry_order: the slots pos*K+code in stored order (None: position-major)"""
        cb = _f32(codebook)
        m, K, s = cb.shape
        od = np.arange(m * K) if entry_order is None else np.asarray(entry_order)
        pos, code = _i32(od // K), _i32(od % K)
        vec = _f32(cb.reshape(m * K, s)[od])
        self._ck(self.lib.fr_add_codebook(table.encode(), m * K, s, _p(pos), _p(code), _p(vec)))

    def add_vectors(self, table, ids, vectors):
        ids, v = _i32(ids), _f32(vectors)
        self._ck(self.lib.fr_add_id_vector(table.encode(), C.c_int64(ids.size), v.shape[1], _p(ids), _p(v), None))

    def add_pq_rows(self, ids, codes):
        ids, c = _i32(ids), _i16(codes)
        self._ck(self.lib.fr_add_id_vector(b"pq_quantization", C.c_int64(ids.size), c.shape[1], _p(ids), None, _p(c)))

    def add_fine_rows(self, ids, coarse_id, codes):
        ids, cid, c = _i32(ids), _i32(coarse_id), _i16(codes)
        self._ck(self.lib.fr_add_fine(b"fine_quantization", C.c_int64(ids.size), c.shape[1], _p(ids), _p(cid), _p(c)))

    def spi(self, command, max_rows=4096):
        """(row count, first column as int32) of a statement run by the stand-in SPI"""
        rows = C.c_int64()
        first = np.zeros(max_rows, np.int32)
        self._ck(self.lib.fr_spi_count(command.encode(), C.byref(rows), _p(first), max_rows))
        return rows.value, first[:min(rows.value, max_rows)]

    # ---- SRFs ------------------------------------------------------------------------------------------
    @staticmethod
    def _strs(buf, rows, ncols):
        return [[buf[(r * ncols + c) * STRLEN:(r * ncols + c + 1) * STRLEN].split(b"\0")[0].decode() for c in range(ncols)]
                for r in range(rows)]

    def _single(self, fn, k, *args):
        out = np.empty(k, ENTRY)
        buf = C.create_string_buffer(k * 2 * STRLEN)
        rows = C.c_int64()
        self._ck(fn(*args, _p(out), buf, C.byref(rows)))
        return out, self._strs(buf.raw, rows.value, 2)

    def pq_search(self, q, k):
        q = _f32(q)
        return self._single(self.lib.fr_srf_pq_search, k, _p(q), q.size, k)

    def pq_search_in(self, q, k, input_ids):
        q, ids = _f32(q), _i32(input_ids)
        return self._single(self.lib.fr_srf_pq_search_in, k, _p(q), q.size, k, _p(ids), ids.size)

    def ivfadc_search(self, q, k):
        q = _f32(q)
        return self._single(self.lib.fr_srf_ivfadc_search, k, _p(q), q.size, k)

    def ivfadc_batch_search(self, query_ids, k):
        """(query ids in fetch order, entries [Q][k], emitted rows)"""
        ids = _i32(query_ids)
        out = np.empty((ids.size, k), ENTRY)
        qid = np.empty(ids.size, np.int32)
        buf = C.create_string_buffer(ids.size * k * 3 * STRLEN)
        rows, nq = C.c_int64(), C.c_int()
        self._ck(self.lib.fr_srf_ivfadc_batch_search(_p(ids), ids.size, k, _p(qid), _p(out), buf, C.byref(rows), C.byref(nq)))
        return qid[:nq.value], out[:nq.value], self._strs(buf.raw, rows.value, 3)

    def grouping_pq(self, input_ids, group_ids):
        """(ids, index into the sorted group ids, sorted group ids, emitted rows)"""
        ids, g = _i32(input_ids), _i32(group_ids)
        oi, og, sg = np.empty(max(ids.size, 1), np.int32), np.empty(max(ids.size, 1), np.int32), np.empty(g.size, np.int32)
        buf = C.create_string_buffer(max(ids.size, 1) * 2 * STRLEN)
        rows = C.c_int64()
        self._ck(self.lib.fr_srf_grouping_pq(_p(ids), ids.size, _p(g), g.size, _p(oi), _p(og), _p(sg), buf, C.byref(rows)))
        return oi[:rows.value], og[:rows.value], sg, self._strs(buf.raw, rows.value, 2)
