"""What the entry points of exact.hip, analogy.hip, rerank.hip, cluster.hip, similarity.hip and tokenize.hip refuse, and in which order:
a fixed list of refused calls is replayed against the built library, and every return code and freddy_gpu_last_error() text is
compared with tests/golden/exact_refusals.json, which was recorded from the library of the commit before the units were split
(when all of them were one exact.hip).  Where an entry point can refuse two things at once a call has both wrong: the order is pinned.

"cpu": refused before any handle is read -- NULL handles, or (`dummy`) a non-NULL pointer to zeros where the refusal comes before the
entry point looks at the handle.  No device is opened.  "gpu": a handle of the wrong kind for every handle argument (a vector table
of 64 rows and a pq table of d = 64, m = 8, K = 128, 64 rows), and the scalar refusals of the entry points that look at their handle
first; no kernel is launched beyond the two pins.

Recording (with the library of the commit the golden file is to describe):
    FREDDY_GPU_SO=<libfreddy_gpu.so> python tests/test_exact_refusals_cpu.py cpu|gpu <out.json>"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exact_refusals.json")
NAN = float("nan")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Bufs:
    """the arguments of the calls: small arrays that nothing writes (every call is refused)"""

    def __init__(self):
        self.q = np.zeros((2, 64), np.float32)
        self.ids = np.array([1, 2, 3], np.int32)
        self.tri = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
        self.oi = np.zeros(64, np.int32)
        self.of = np.zeros(64, np.float32)
        self.od = np.zeros(64, np.float64)
        self.ob = np.zeros(64, np.uint8)
        self.n = np.zeros(1, np.int32)
        self.n64 = np.zeros(1, np.int64)
        self.draws = np.full(64, 0.5, np.float64)
        self.nan_draws = np.array([0.5, NAN, 0.5, 0.5], np.float64)
        self.off = np.array([0, 1, 3], np.int64)
        self.off_from_one = np.array([1, 2, 3], np.int64)
        self.off_down = np.array([0, 2, 1], np.int64)
        self.off_long = np.array([0, 4097], np.int64)
        self.tok_long = np.ones(4097, np.int32)
        self.zeros = np.zeros(1 << 16, np.uint8)   # `dummy`


def cpu_calls(lib, b):
    """[(name, thunk -> rc)]: refused before a handle is read"""
    from freddy_amd import gpu
    null = None
    dummy = _p(b.zeros)
    q, ids, tri, oi, of, od, ob = _p(b.q), _p(b.ids), _p(b.tri), _p(b.oi), _p(b.of), _p(b.od), _p(b.ob)
    n, n64, draws, off = _p(b.n), _p(b.n64), _p(b.draws), _p(b.off)
    out = C.c_void_p()
    calls = []

    def add(name, fn):
        calls.append((name, fn))

    # ---- exact.hip
    def pin(d, N, id_values=(1, 2)):
        row_ids = np.array(id_values, np.int32)
        desc = gpu.VecDesc(d, N, _p(row_ids), q)
        return lambda row_ids=row_ids: lib.freddy_gpu_pin_vectors(C.byref(desc), 0, C.byref(out))
    add("pin_vectors/null_desc", lambda: lib.freddy_gpu_pin_vectors(null, 0, C.byref(out)))
    add("pin_vectors/null_out", lambda: lib.freddy_gpu_pin_vectors(C.byref(gpu.VecDesc(4, 2, ids, q)), 0, null))
    add("pin_vectors/d=0", pin(0, 2))
    add("pin_vectors/N<0", pin(4, -1))
    add("pin_vectors/N_too_large", pin(4, (1 << 31) - 64))
    add("pin_vectors/d_too_large", pin(5000, 2))
    add("pin_vectors/N_and_d_too_large", pin(5000, (1 << 31) - 64))
    add("pin_vectors/ids_not_ascending", pin(4, 2, (2, 2)))
    add("pin_vectors/d_too_large+ids_not_ascending", pin(5000, 2, (2, 2)))
    add("exact_search/null", lambda: lib.freddy_gpu_exact_search(null, q, 2, 3, null, 0, oi, of))
    add("exact_search/null+k=4097+Q<0", lambda: lib.freddy_gpu_exact_search(null, q, -1, 4097, null, 0, oi, of))

    def search_ids(vecs=dummy, query_ids=ids, n_ids=2, rule=0, k=3, sub=null, n_sub=0, oq=oi, nq=n, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_exact_search_ids(vecs, query_ids, n_ids, rule, k, sub, n_sub, oq, nq, o_i, o_s)
    add("exact_search_ids/null", search_ids(vecs=null))
    add("exact_search_ids/null+n_ids<0", search_ids(vecs=null, n_ids=-1))
    add("exact_search_ids/n_ids<0", search_ids(n_ids=-1))
    add("exact_search_ids/id_rule", search_ids(rule=2))
    add("exact_search_ids/n_ids<0+id_rule", search_ids(n_ids=-1, rule=2))
    add("exact_search_ids/null_n_queries", search_ids(nq=null))
    add("exact_search_ids/null_buffer", search_ids(query_ids=null))
    add("exact_search_ids/k=0", search_ids(k=0))
    add("exact_search_ids/n_subset<0", search_ids(n_sub=-1))
    add("exact_search_ids/null_subset", search_ids(n_sub=1))
    add("exact_search_ids/k=4097", search_ids(k=4097))
    add("exact_search_ids/k=4097+n_subset<0", search_ids(k=4097, n_sub=-1))
    add("exact_search_ids/k=4097+null_buffer", search_ids(k=4097, o_i=null))

    def join(ix=null, queries=q, Q=2, k=3, t=ids, nt=3, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_exact_join(ix, queries, Q, k, t, nt, o_i, o_s)
    add("exact_join/null", join())
    add("exact_join/Q<0", join(Q=-1))
    add("exact_join/k=0", join(k=0))
    add("exact_join/n_targets<0", join(nt=-1))
    add("exact_join/null_targets", join(t=null))
    add("exact_join/null_buffer", join(queries=null))
    add("exact_join/k=4097", join(k=4097))
    add("exact_join/k=4097+null_buffer", join(k=4097, o_s=null))
    add("exact_join/k=4097+null_targets", join(k=4097, t=null))
    add("exact_join/k=0+null_targets", join(k=0, t=null))

    def join_ids(vecs=dummy, query_ids=ids, n_ids=2, rule=0, k=3, t=ids, nt=3, oq=oi, nq=n, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_exact_join_ids(vecs, query_ids, n_ids, rule, k, t, nt, oq, nq, o_i, o_s)
    add("exact_join_ids/null", join_ids(vecs=null))
    add("exact_join_ids/n_ids<0", join_ids(n_ids=-1))
    add("exact_join_ids/id_rule", join_ids(rule=-1))
    add("exact_join_ids/null_n_queries", join_ids(nq=null))
    add("exact_join_ids/null_buffer", join_ids(oq=null))
    add("exact_join_ids/k=0", join_ids(k=0))
    add("exact_join_ids/n_targets<0", join_ids(nt=-1))
    add("exact_join_ids/null_targets", join_ids(t=null))
    add("exact_join_ids/k=4097", join_ids(k=4097))
    add("exact_join_ids/k=4097+null_targets", join_ids(k=4097, t=null))
    add("exact_join_ids/k=4097+id_rule", join_ids(k=4097, rule=5))
    add("debug_resolve_ids/null", lambda: lib.freddy_gpu_debug_resolve_ids(null, ids, 3, oi, n64))
    add("debug_resolve_ids/n<0", lambda: lib.freddy_gpu_debug_resolve_ids(dummy, ids, -1, oi, n64))
    add("debug_resolve_ids/null_n_rows", lambda: lib.freddy_gpu_debug_resolve_ids(dummy, ids, 3, oi, null))
    add("debug_resolve_ids/null_ids", lambda: lib.freddy_gpu_debug_resolve_ids(dummy, null, 3, oi, n64))
    add("debug_resolve_ids/null+n<0", lambda: lib.freddy_gpu_debug_resolve_ids(null, ids, -1, oi, n64))
    add("last_exact_join_stats/null", lambda: lib.freddy_gpu_last_exact_join_stats(null, n64, n64, n64))

    # ---- analogy.hip
    def analogy(ix=null, method=0, t=tri, Q=2, k=3, sub=null, n_sub=0, o_i=oi, o_s=od):
        return lambda: lib.freddy_gpu_exact_analogy(ix, method, t, Q, k, sub, n_sub, o_i, o_s)
    add("exact_analogy/null", analogy())
    add("exact_analogy/method", analogy(method=7))
    add("exact_analogy/Q<0", analogy(Q=-1))
    add("exact_analogy/k=0", analogy(k=0))
    add("exact_analogy/n_subset<0", analogy(n_sub=-1))
    add("exact_analogy/null_subset", analogy(n_sub=2))
    add("exact_analogy/null_buffer", analogy(t=null))
    add("exact_analogy/k=33", analogy(k=33))
    add("exact_analogy/k=4097", analogy(k=4097))
    add("exact_analogy/method+k=4097", analogy(method=-1, k=4097))
    add("exact_analogy/k=4097+null_buffer", analogy(k=4097, o_s=null))
    add("last_analogy_stats/null", lambda: lib.freddy_gpu_last_analogy_stats(null, n64, n64, n64))

    # ---- rerank.hip
    def ivf_pv(ivf=null, vecs=null, queries=q, Q=2, k=3, pvf=2, W=2, rule=0, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_ivfadc_search_pv(ivf, vecs, queries, Q, k, pvf, W, 1000.0, rule, o_i, o_s)
    add("ivfadc_search_pv/null", ivf_pv())
    add("ivfadc_search_pv/null_vecs", ivf_pv(ivf=dummy))
    add("ivfadc_search_pv/Q<0", ivf_pv(Q=-1))
    add("ivfadc_search_pv/k=0", ivf_pv(k=0))
    add("ivfadc_search_pv/pvf=0", ivf_pv(pvf=0))
    add("ivfadc_search_pv/null_buffer", ivf_pv(queries=null))
    add("ivfadc_search_pv/k=4097", ivf_pv(k=4097, pvf=1))
    add("ivfadc_search_pv/k*pvf=4100", ivf_pv(k=1025, pvf=4))
    add("ivfadc_search_pv/k=4097+null_buffer", ivf_pv(k=4097, o_i=null))
    add("ivfadc_search_pv/null+W=0", ivf_pv(W=0))

    def pq_pv(pq=null, vecs=null, queries=q, Q=2, k=3, pvf=2, sub=null, n_sub=0, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_pq_search_pv(pq, vecs, queries, Q, k, pvf, 100.0, sub, n_sub, o_i, o_s)
    add("pq_search_pv/null", pq_pv())
    add("pq_search_pv/n_subset<0", pq_pv(n_sub=-1))
    add("pq_search_pv/null_subset", pq_pv(n_sub=2))
    add("pq_search_pv/Q<0", pq_pv(Q=-1))
    add("pq_search_pv/n_subset<0+Q<0", pq_pv(n_sub=-1, Q=-1))
    add("pq_search_pv/null_buffer", pq_pv(o_s=null))
    add("pq_search_pv/k=4097", pq_pv(k=4097, pvf=1))

    def ivf_pv_ids(ivf=dummy, vecs=dummy, query_ids=ids, n_ids=2, rule=0, k=3, pvf=2, W=2, found=0, oq=oi, nq=n, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_ivfadc_search_pv_ids(ivf, vecs, query_ids, n_ids, rule, k, pvf, W, 1000.0, found, oq, nq, o_i, o_s)
    add("ivfadc_search_pv_ids/null", ivf_pv_ids(ivf=null))
    add("ivfadc_search_pv_ids/null_vecs", ivf_pv_ids(vecs=null))
    add("ivfadc_search_pv_ids/n_ids<0", ivf_pv_ids(n_ids=-1))
    add("ivfadc_search_pv_ids/id_rule", ivf_pv_ids(rule=2))
    add("ivfadc_search_pv_ids/null_n_queries", ivf_pv_ids(nq=null))
    add("ivfadc_search_pv_ids/null_buffer", ivf_pv_ids(o_i=null))
    add("ivfadc_search_pv_ids/k=0", ivf_pv_ids(k=0))
    add("ivfadc_search_pv_ids/pvf=0", ivf_pv_ids(pvf=0))
    add("ivfadc_search_pv_ids/k=4097", ivf_pv_ids(k=4097, pvf=1))
    add("ivfadc_search_pv_ids/W=0", ivf_pv_ids(W=0))
    add("ivfadc_search_pv_ids/found_rule", ivf_pv_ids(found=3))
    add("ivfadc_search_pv_ids/batch_udf_W=2", ivf_pv_ids(found=2))
    add("ivfadc_search_pv_ids/k=4097+W=0", ivf_pv_ids(k=4097, pvf=1, W=0))
    add("ivfadc_search_pv_ids/id_rule+k=0", ivf_pv_ids(rule=2, k=0))

    def pq_pv_ids(pq=dummy, vecs=dummy, query_ids=ids, n_ids=2, rule=0, k=3, pvf=2, sub=null, n_sub=0, oq=oi, nq=n, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_pq_search_pv_ids(pq, vecs, query_ids, n_ids, rule, k, pvf, 100.0, sub, n_sub, oq, nq, o_i, o_s)
    add("pq_search_pv_ids/null", pq_pv_ids(pq=null))
    add("pq_search_pv_ids/n_ids<0", pq_pv_ids(n_ids=-1))
    add("pq_search_pv_ids/null_buffer", pq_pv_ids(query_ids=null))
    add("pq_search_pv_ids/n_subset<0", pq_pv_ids(n_sub=-1))
    add("pq_search_pv_ids/k=0", pq_pv_ids(k=0))
    add("pq_search_pv_ids/n_subset<0+k=0", pq_pv_ids(n_sub=-1, k=0))
    add("pq_search_pv_ids/k=4097", pq_pv_ids(k=4097, pvf=1))
    add("pq_search_pv_ids/k=0+k*pvf", pq_pv_ids(k=0, pvf=5000))
    add("last_pv_stats/null", lambda: lib.freddy_gpu_last_pv_stats(null, n64, n64))

    def ivf_an(ivf=null, vecs=null, t=tri, Q=2, k=3, n_cand=8, W=2, found=0, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_ivfadc_analogy(ivf, vecs, t, Q, k, n_cand, W, 1000.0, found, o_i, o_s)
    add("ivfadc_analogy/null", ivf_an())
    add("ivfadc_analogy/W=0", ivf_an(W=0))
    add("ivfadc_analogy/found_rule", ivf_an(found=-1))
    add("ivfadc_analogy/Q<0", ivf_an(Q=-1))
    add("ivfadc_analogy/n_cand<k", ivf_an(k=9))
    add("ivfadc_analogy/null_buffer", ivf_an(t=null))
    add("ivfadc_analogy/n_cand=4097", ivf_an(n_cand=4097))
    add("ivfadc_analogy/k=4097", ivf_an(k=4097, n_cand=4097))
    add("ivfadc_analogy/W=0+Q<0", ivf_an(W=0, Q=-1))

    def pq_an(pq=null, vecs=null, t=tri, Q=2, k=3, n_cand=8, sub=null, n_sub=0, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_pq_analogy(pq, vecs, t, Q, k, n_cand, 100.0, sub, n_sub, o_i, o_s)
    add("pq_analogy/null", pq_an())
    add("pq_analogy/null_vecs", pq_an(pq=dummy))
    add("pq_analogy/n_subset<0", pq_an(n_sub=-1))
    add("pq_analogy/k=0", pq_an(k=0))
    add("pq_analogy/n_subset<0+k=0", pq_an(n_sub=-1, k=0))
    add("pq_analogy/null_buffer", pq_an(o_i=null))
    add("pq_analogy/n_cand=4097", pq_an(n_cand=4097))
    add("pq_analogy/k=4097", pq_an(k=4097, n_cand=4097))

    def ivpq_an(ivpq=null, vecs=null, t=tri, Q=2, k=3, n_cand=4, tg=ids, nt=3, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_ivpq_analogy(ivpq, vecs, t, Q, k, n_cand, tg, nt, 1, 1, 0, 0, 0.8, 0, o_i, o_s)
    add("ivpq_analogy/null", ivpq_an())
    add("ivpq_analogy/null_vecs", ivpq_an(ivpq=dummy))
    add("ivpq_analogy/Q<0", ivpq_an(Q=-1))
    add("ivpq_analogy/n_cand<k", ivpq_an(k=5))
    add("ivpq_analogy/null_buffer", ivpq_an(o_s=null))
    add("ivpq_analogy/n_cand=4097", ivpq_an(n_cand=4097))
    add("ivpq_analogy/k=4097", ivpq_an(k=4097, n_cand=4097))
    add("last_approx_analogy_stats/null", lambda: lib.freddy_gpu_last_approx_analogy_stats(null, n64, n64, n64))

    # ---- cluster.hip
    def assign(ix=null, queries=q, Q=2, t=ids, nt=3, o_q=oi, o_s=of):
        return lambda: lib.freddy_gpu_exact_assign(ix, queries, Q, t, nt, o_q, o_s)
    add("exact_assign/null", assign())
    add("exact_assign/Q<0", assign(Q=-1))
    add("exact_assign/n_targets<0", assign(nt=-1))
    add("exact_assign/null_buffer", assign(t=null))
    add("exact_assign/Q=65537", assign(Q=65537))
    add("exact_assign/Q=65537+null_buffer", assign(Q=65537, o_q=null))
    add("exact_assign/null+Q=0", assign(Q=0))

    def cluster(vecs=null, pq=null, sentinel=100.0, t=ids, n_tok=3, kc=2, rounds=2, dr=draws, n_draws=64, o_c=oi):
        return lambda: lib.freddy_gpu_cluster(vecs, pq, sentinel, t, n_tok, kc, rounds, dr, n_draws, o_c, of, null)
    add("cluster/null", cluster())
    add("cluster/n=0", cluster(n_tok=0))
    add("cluster/kc=0", cluster(kc=0))
    add("cluster/rounds=0", cluster(rounds=0))
    add("cluster/null_buffer", cluster(dr=null))
    add("cluster/kc=65537", cluster(kc=65537))
    add("cluster/n>int32", cluster(n_tok=1 << 31))
    add("cluster/kc=65537+n>int32", cluster(kc=65537, n_tok=1 << 31))
    add("cluster/n_draws", cluster(n_draws=21))
    add("cluster/nan_draw", cluster(dr=_p(b.nan_draws), kc=2, rounds=1, n_draws=4))
    add("cluster/sentinel_nan", cluster(pq=dummy, sentinel=NAN))
    add("cluster/sentinel_large", cluster(pq=dummy, sentinel=3.0e7))
    add("cluster/sentinel_nan_without_pq", cluster(sentinel=NAN))
    add("cluster/n_draws+sentinel_nan", cluster(pq=dummy, sentinel=NAN, n_draws=21))

    # ---- similarity.hip
    add("similarity_pairs/null", lambda: lib.freddy_gpu_similarity_pairs(null, ids, ids, 3, of, ob))
    add("similarity_pairs/n<0", lambda: lib.freddy_gpu_similarity_pairs(null, ids, ids, -1, of, ob))
    add("similarity_pairs/null_buffer", lambda: lib.freddy_gpu_similarity_pairs(null, ids, null, 3, of, ob))
    add("similarity_pairs/null+n=0", lambda: lib.freddy_gpu_similarity_pairs(null, ids, ids, 0, of, ob))

    def matrix(ix=null, a_ids=ids, a_vec=null, na=3, b_ids=ids, nb=3, o=of, ka=ob, kb=ob):
        return lambda: lib.freddy_gpu_similarity_matrix(ix, a_ids, a_vec, na, b_ids, nb, o, ka, kb)
    add("similarity_matrix/null", matrix())
    add("similarity_matrix/na<0", matrix(na=-1))
    add("similarity_matrix/nb<0", matrix(nb=-1))
    add("similarity_matrix/both_sides", matrix(a_vec=q))
    add("similarity_matrix/no_side", matrix(a_ids=null))
    add("similarity_matrix/null_b", matrix(b_ids=null))
    add("similarity_matrix/nb_limit", matrix(nb=(1 << 22) + 1))
    add("similarity_matrix/null_buffer", matrix(o=null))
    add("similarity_matrix/na<0+both_sides", matrix(na=-1, a_vec=q))
    add("similarity_matrix/nb_limit+null_buffer", matrix(nb=(1 << 22) + 1, ka=null))

    def sjoin(ix=null, a_ids=ids, a_vec=null, na=3, b_ids=ids, nb=3, max_pairs=8, o_a=oi, o_b=oi, o_s=of, n_pairs=n64):
        return lambda: lib.freddy_gpu_similarity_join(ix, a_ids, a_vec, na, b_ids, nb, 0.5, max_pairs, o_a, o_b, o_s, n_pairs)
    add("similarity_join/null", sjoin())
    add("similarity_join/na<0", sjoin(na=-1))
    add("similarity_join/both_sides", sjoin(a_vec=q))
    add("similarity_join/null_b", sjoin(b_ids=null))
    add("similarity_join/nb_limit", sjoin(nb=(1 << 22) + 1))
    add("similarity_join/max_pairs<0", sjoin(max_pairs=-1))
    add("similarity_join/null_n_pairs", sjoin(n_pairs=null))
    add("similarity_join/null_buffer", sjoin(o_b=null))
    add("similarity_join/max_pairs<0+null_n_pairs", sjoin(max_pairs=-1, n_pairs=null))
    add("similarity_join/nb_limit+max_pairs<0", sjoin(nb=(1 << 22) + 1, max_pairs=-1))

    # ---- tokenize.hip
    def tok(vecs=null, t=ids, o=off, n_texts=2, rule=0, o_v=of, o_c=oi):
        return lambda: lib.freddy_gpu_tokenize(vecs, t, o, n_texts, rule, 1, o_v, o_c)
    add("tokenize/null", tok())
    add("tokenize/null_out_vectors", tok(o_v=null))
    add("tokenize/n_texts<0", tok(n_texts=-1))
    add("tokenize/id_rule", tok(rule=2))
    add("tokenize/null_offsets", tok(o=null))
    add("tokenize/null_out_count", tok(o_c=null))
    add("tokenize/offsets_from_one", tok(o=_p(b.off_from_one)))
    add("tokenize/offsets_decrease", tok(o=_p(b.off_down)))
    add("tokenize/null_token_ids", tok(t=null))
    add("tokenize/text_too_long", tok(t=_p(b.tok_long), o=_p(b.off_long), n_texts=1))
    add("tokenize/null_out_vectors+id_rule", tok(o_v=null, rule=2))
    add("tokenize/null+n_texts=0", tok(n_texts=0))

    def ivf_texts(ivf=null, vecs=null, t=ids, o=off, n_texts=2, rule=0, k=3, W=2, found=0, o_c=oi, o_i=oi, o_d=of):
        return lambda: lib.freddy_gpu_ivfadc_search_texts(ivf, vecs, t, o, n_texts, rule, k, W, 1000.0, found, o_c, o_i, o_d)
    add("ivfadc_search_texts/null", ivf_texts())
    add("ivfadc_search_texts/k=0", ivf_texts(k=0))
    add("ivfadc_search_texts/null_buffer", ivf_texts(o_i=null))
    add("ivfadc_search_texts/W=0", ivf_texts(W=0))
    add("ivfadc_search_texts/found_rule", ivf_texts(found=3))
    add("ivfadc_search_texts/n_texts<0", ivf_texts(n_texts=-1))
    add("ivfadc_search_texts/offsets_decrease", ivf_texts(o=_p(b.off_down)))
    add("ivfadc_search_texts/text_too_long", ivf_texts(t=_p(b.tok_long), o=_p(b.off_long), n_texts=1))
    add("ivfadc_search_texts/k=4097", ivf_texts(k=4097))
    add("ivfadc_search_texts/k=0+W=0", ivf_texts(k=0, W=0))
    add("ivfadc_search_texts/W=0+id_rule", ivf_texts(W=0, rule=2))
    add("ivfadc_search_texts/k=4097+id_rule", ivf_texts(k=4097, rule=2))
    add("ivfadc_search_texts/k=4097+text_too_long", ivf_texts(k=4097, t=_p(b.tok_long), o=_p(b.off_long), n_texts=1))

    def pq_texts(pq=null, vecs=null, t=ids, o=off, n_texts=2, rule=0, k=3, sub=null, n_sub=0, o_c=oi, o_i=oi, o_d=of):
        return lambda: lib.freddy_gpu_pq_search_texts(pq, vecs, t, o, n_texts, rule, k, 100.0, sub, n_sub, o_c, o_i, o_d)
    add("pq_search_texts/null", pq_texts())
    add("pq_search_texts/k=0", pq_texts(k=0))
    add("pq_search_texts/null_buffer", pq_texts(o_d=null))
    add("pq_search_texts/n_subset<0", pq_texts(n_sub=-1))
    add("pq_search_texts/null_subset", pq_texts(n_sub=2))
    add("pq_search_texts/id_rule", pq_texts(rule=2))
    add("pq_search_texts/k=4097", pq_texts(k=4097))
    add("pq_search_texts/k=0+n_subset<0", pq_texts(k=0, n_sub=-1))
    add("pq_search_texts/n_subset<0+id_rule", pq_texts(n_sub=-1, rule=2))
    add("pq_search_texts/k=4097+offsets_from_one", pq_texts(k=4097, o=_p(b.off_from_one)))

    def exact_texts(vecs=null, t=ids, o=off, n_texts=2, rule=0, k=3, sub=null, n_sub=0, o_c=oi, o_i=oi, o_s=of):
        return lambda: lib.freddy_gpu_exact_search_texts(vecs, t, o, n_texts, rule, 1, k, sub, n_sub, o_c, o_i, o_s)
    add("exact_search_texts/null", exact_texts())
    add("exact_search_texts/k=0", exact_texts(k=0))
    add("exact_search_texts/null_buffer", exact_texts(o_i=null))
    add("exact_search_texts/n_subset<0", exact_texts(n_sub=-1))
    add("exact_search_texts/n_texts<0", exact_texts(n_texts=-1))
    add("exact_search_texts/null_out_count", exact_texts(o_c=null))
    add("exact_search_texts/k=4097", exact_texts(k=4097))
    add("exact_search_texts/k=4097+n_subset<0", exact_texts(k=4097, n_sub=-1))
    add("exact_search_texts/k=4097+n_texts<0", exact_texts(k=4097, n_texts=-1))
    return calls


def gpu_calls(lib, b, V, P):
    """[(name, thunk -> rc)]: V a pinned vector table, P a pinned pq table of the same d; every call hands one of them to an
    argument that wants the other kind (or an ivf / ivpq handle), or asks a handle-first entry point for something it refuses."""
    q, ids, tri, oi, of, od, ob = _p(b.q), _p(b.ids), _p(b.tri), _p(b.oi), _p(b.of), _p(b.od), _p(b.ob)
    n, n64, draws, off = _p(b.n), _p(b.n64), _p(b.draws), _p(b.off)
    null = None
    calls = []

    def add(name, fn):
        calls.append((name, fn))

    # ---- a pq handle where a vector handle is wanted
    add("exact_search/pq", lambda: lib.freddy_gpu_exact_search(P, q, 2, 3, null, 0, oi, of))
    add("exact_search/pq+k=4097", lambda: lib.freddy_gpu_exact_search(P, q, 2, 4097, null, 0, oi, of))
    add("exact_search_ids/pq", lambda: lib.freddy_gpu_exact_search_ids(P, ids, 2, 0, 3, null, 0, oi, n, oi, of))
    add("exact_search_ids/pq+k=4097", lambda: lib.freddy_gpu_exact_search_ids(P, ids, 2, 0, 4097, null, 0, oi, n, oi, of))
    add("exact_join/pq", lambda: lib.freddy_gpu_exact_join(P, q, 2, 3, ids, 3, oi, of))
    add("exact_join/pq+k=4097", lambda: lib.freddy_gpu_exact_join(P, q, 2, 4097, ids, 3, oi, of))
    add("exact_join_ids/pq", lambda: lib.freddy_gpu_exact_join_ids(P, ids, 2, 0, 3, ids, 3, oi, n, oi, of))
    add("debug_resolve_ids/pq", lambda: lib.freddy_gpu_debug_resolve_ids(P, ids, 3, oi, n64))
    add("last_exact_join_stats/pq", lambda: lib.freddy_gpu_last_exact_join_stats(P, n64, n64, n64))
    add("exact_analogy/pq", lambda: lib.freddy_gpu_exact_analogy(P, 0, tri, 2, 3, null, 0, oi, od))
    add("last_analogy_stats/pq", lambda: lib.freddy_gpu_last_analogy_stats(P, n64, n64, n64))
    add("exact_assign/pq", lambda: lib.freddy_gpu_exact_assign(P, q, 2, ids, 3, oi, of))
    add("cluster/pq_as_vecs", lambda: lib.freddy_gpu_cluster(P, null, 100.0, ids, 3, 2, 2, draws, 64, oi, of, null))
    add("cluster/vecs_as_pq", lambda: lib.freddy_gpu_cluster(V, V, 100.0, ids, 3, 2, 2, draws, 64, oi, of, null))
    add("similarity_pairs/pq", lambda: lib.freddy_gpu_similarity_pairs(P, ids, ids, 3, of, ob))
    add("similarity_matrix/pq", lambda: lib.freddy_gpu_similarity_matrix(P, ids, null, 3, ids, 3, of, ob, ob))
    add("similarity_join/pq", lambda: lib.freddy_gpu_similarity_join(P, ids, null, 3, ids, 3, 0.5, 8, oi, oi, of, n64))
    add("tokenize/pq", lambda: lib.freddy_gpu_tokenize(P, ids, off, 2, 0, 1, of, oi))
    add("exact_search_texts/pq", lambda: lib.freddy_gpu_exact_search_texts(P, ids, off, 2, 0, 1, 3, null, 0, oi, oi, of))
    # ---- the two-handle calls: the vector handle where the pq / ivf / ivpq handle is wanted, the pq handle where the vectors are
    for name, ann, vecs in (("vecs_as_ann", V, V), ("pq_as_vecs", P, P), ("swapped", V, P)):
        add("pq_search_pv/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_pq_search_pv(ann, vecs, q, 2, 3, 2, 100.0, null, 0, oi, of))
        add("pq_search_pv_ids/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_pq_search_pv_ids(ann, vecs, ids, 2, 0, 3, 2, 100.0, null, 0, oi, n, oi, of))
        add("pq_analogy/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_pq_analogy(ann, vecs, tri, 2, 3, 8, 100.0, null, 0, oi, of))
        add("pq_search_texts/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_pq_search_texts(ann, vecs, ids, off, 2, 0, 3, 100.0, null, 0, oi, oi, of))
    for name, ann, vecs in (("vecs_as_ivf", V, V), ("pq_as_ivf", P, V), ("pq_as_both", P, P)):
        add("ivfadc_search_pv/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_ivfadc_search_pv(ann, vecs, q, 2, 3, 2, 2, 1000.0, 0, oi, of))
        add("ivfadc_search_pv_ids/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_ivfadc_search_pv_ids(ann, vecs, ids, 2, 0, 3, 2, 2, 1000.0, 0, oi, n, oi, of))
        add("ivfadc_analogy/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_ivfadc_analogy(ann, vecs, tri, 2, 3, 8, 2, 1000.0, 0, oi, of))
        add("ivfadc_search_texts/" + name, lambda ann=ann, vecs=vecs: lib.freddy_gpu_ivfadc_search_texts(ann, vecs, ids, off, 2, 0, 3, 2, 1000.0, 0, oi, oi, of))
    add("ivfadc_search_pv/pq_as_ivf+W=0", lambda: lib.freddy_gpu_ivfadc_search_pv(P, V, q, 2, 3, 2, 0, 1000.0, 0, oi, of))
    add("last_pv_stats/vecs", lambda: lib.freddy_gpu_last_pv_stats(V, n64, n64))
    add("last_approx_analogy_stats/vecs", lambda: lib.freddy_gpu_last_approx_analogy_stats(V, n64, n64, n64))
    # ---- what the entry points that look at their handle first refuse behind it (the right handle; nothing is launched)
    add("exact_search/Q<0", lambda: lib.freddy_gpu_exact_search(V, q, -1, 3, null, 0, oi, of))
    add("exact_search/k=0", lambda: lib.freddy_gpu_exact_search(V, q, 2, 0, null, 0, oi, of))
    add("exact_search/null_subset", lambda: lib.freddy_gpu_exact_search(V, q, 2, 3, null, 2, oi, of))
    add("exact_search/null_buffer", lambda: lib.freddy_gpu_exact_search(V, null, 2, 3, null, 0, oi, of))
    add("exact_search/k=4097", lambda: lib.freddy_gpu_exact_search(V, q, 2, 4097, null, 0, oi, of))
    add("exact_search/k=4097+null_buffer", lambda: lib.freddy_gpu_exact_search(V, q, 2, 4097, null, 0, null, of))
    add("exact_search/k=4097+n_subset<0", lambda: lib.freddy_gpu_exact_search(V, q, 2, 4097, null, -1, oi, of))
    add("pq_search_pv/W_irrelevant_k*pvf", lambda: lib.freddy_gpu_pq_search_pv(P, V, q, 2, 1025, 4, 100.0, null, 0, oi, of))
    add("ivfadc_search_texts/pq_as_ivf+k=4097", lambda: lib.freddy_gpu_ivfadc_search_texts(P, V, ids, off, 2, 0, 4097, 2, 1000.0, 0, oi, oi, of))
    return calls


def replay(lib, calls):
    """{name: [rc, message]}"""
    got = {}
    for name, fn in calls:
        assert name not in got, name
        rc = fn()
        got[name] = [int(rc), lib.freddy_gpu_last_error().decode() if rc else ""]
    return got


def _pin_two(gpu):
    rng = np.random.default_rng(7)
    ids = np.arange(1, 65, dtype=np.int32)
    V = gpu.VectorIndex(ids, rng.standard_normal((64, 64)).astype(np.float32), device=0)
    P = gpu.PQIndex(rng.standard_normal((8, 128, 8)).astype(np.float32), ids, rng.integers(0, 128, (64, 8)).astype(np.int16), device=0)
    return V, P


def _compare(got, want):
    assert list(got) == list(want), "the list of calls and the golden file differ: record it again from the commit it describes"
    for name in want:
        print(name, got[name])
        assert got[name] == want[name], (name, got[name], want[name])
        assert got[name][0] != 0, (name, "the call was not refused")


def test_refusals_before_any_handle_is_read():
    from freddy_amd import gpu
    lib = gpu.load()
    want = json.load(open(GOLDEN))["cpu"]
    b = _Bufs()
    _compare(replay(lib, cpu_calls(lib, b)), want)
    for a in (b.oi, b.of, b.od, b.ob, b.n, b.n64, b.zeros):
        assert not a.any()   # nothing was written
    # every entry point of the six units has at least one call
    heads = {name.split("/")[0] for name in want}
    assert heads == {n[len("freddy_gpu_"):] for n in ENTRY_POINTS}, heads ^ {n[len("freddy_gpu_"):] for n in ENTRY_POINTS}


ENTRY_POINTS = (
    "freddy_gpu_pin_vectors", "freddy_gpu_exact_search", "freddy_gpu_exact_search_ids", "freddy_gpu_exact_join", "freddy_gpu_exact_join_ids",
    "freddy_gpu_debug_resolve_ids", "freddy_gpu_last_exact_join_stats", "freddy_gpu_exact_analogy", "freddy_gpu_last_analogy_stats",
    "freddy_gpu_ivfadc_search_pv", "freddy_gpu_pq_search_pv", "freddy_gpu_ivfadc_search_pv_ids", "freddy_gpu_pq_search_pv_ids", "freddy_gpu_last_pv_stats",
    "freddy_gpu_ivfadc_analogy", "freddy_gpu_pq_analogy", "freddy_gpu_ivpq_analogy", "freddy_gpu_last_approx_analogy_stats",
    "freddy_gpu_exact_assign", "freddy_gpu_cluster", "freddy_gpu_similarity_pairs", "freddy_gpu_similarity_matrix", "freddy_gpu_similarity_join",
    "freddy_gpu_tokenize", "freddy_gpu_ivfadc_search_texts", "freddy_gpu_pq_search_texts", "freddy_gpu_exact_search_texts")


@pytest.mark.gpu
def test_handles_of_the_wrong_kind():
    from freddy_amd import gpu
    lib = gpu.load()
    want = json.load(open(GOLDEN))["gpu"]
    b = _Bufs()
    V, P = _pin_two(gpu)
    try:
        _compare(replay(lib, gpu_calls(lib, b, V.h, P.h)), want)
        # a call with nothing wrong but the kind of a handle ("+": something else is wrong too) is FREDDY_E_KIND with the one message
        only_kind = [name for name in want if "+" not in name and re.search(r"/(pq|vecs|swapped)", name)]
        assert len(only_kind) == 42
        for name in only_kind:
            assert want[name] == [-4, "index handle has the wrong kind for this call"], name
    finally:
        V.close()
        P.close()
    for a in (b.oi, b.of, b.od, b.ob, b.n, b.n64):
        assert not a.any()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu as _gpu
    _lib = _gpu.load()
    _b = _Bufs()
    if sys.argv[1] == "cpu":
        _got = replay(_lib, cpu_calls(_lib, _b))
    else:
        _V, _P = _pin_two(_gpu)
        _got = replay(_lib, gpu_calls(_lib, _b, _V.h, _P.h))
        _V.close()
        _P.close()
    json.dump({sys.argv[1]: _got}, open(sys.argv[2], "w"), indent=0)
    print(len(_got), "calls recorded from", _gpu.LIB_PATH)
