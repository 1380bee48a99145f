"""The kNN-join by row id and the batched analogy over the kNN-join exist in every layer: exported by libfreddy_gpu.so, declared in
include/freddy_gpu.h, listed and bound in freddy_amd/gpu.py, mirrored in freddy_amd/udf.py.  No GPU: the library is loaded and inspected, and
only refusals that are decided before a handle is looked at are provoked."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("freddy_gpu_knn_join_ids", "freddy_gpu_ivpq_analogy")


def test_the_library_exports_them():
    from freddy_amd import gpu
    lib = gpu.load()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes, n
    assert lib.freddy_gpu_abi_version() == 4


def _args(h, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", h)
    assert m, name
    return [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]


def test_the_header_declares_them_and_keeps_its_abi_version():
    h = open(os.path.join(ROOT, "include", "freddy_gpu.h")).read()
    assert _args(h, NAMES[0]) == ["ivpq", "vecs", "query_ids", "n_ids", "id_rule", "k", "target_ids", "n_targets", "alpha", "pvf", "method",
                                  "use_target_lists", "confidence", "double_threshold", "out_query_ids", "n_queries", "out_ids", "out_dist",
                                  "iterations_out"]
    assert _args(h, NAMES[1]) == ["ivpq", "vecs", "triples", "Q", "k", "n_cand", "target_ids", "n_targets", "alpha", "pvf", "method",
                                  "use_target_lists", "confidence", "double_threshold", "out_ids", "out_sim"]
    assert "#define FREDDY_GPU_ABI_VERSION 4" in h
    assert '"join_front_gather"' in h


def test_the_binding_lists_and_wraps_them():
    from freddy_amd import gpu
    lib = gpu.load()
    for n in NAMES:
        assert n in gpu.EXPORTS, n
        assert len(getattr(lib, n).argtypes) == (19 if n == NAMES[0] else 16), n
    for m in ("knn_join_ids", "analogy", "last_approx_analogy_stats"):
        assert callable(getattr(gpu.IVPQIndex, m, None)), m
    assert gpu.ABI_VERSION == 4


def test_refusals_that_need_no_device():
    """NULL handle, n_ids < 0, a bad id_rule, a NULL n_queries: FREDDY_E_ARG with the messages of the other *_ids calls, decided before the
    handle is read (the handle here is a block of zeros, not an index)."""
    from freddy_amd import gpu
    lib = gpu.load()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    q = np.array([1, 2, 3], np.int32)
    tg = np.array([4, 5], np.int32)
    oq, oi, od = np.full(3, -77, np.int32), np.full((3, 5), -77, np.int32), np.full((3, 5), -77.0, np.float32)
    nq, it = C.c_int32(-9), C.c_int32(-9)
    P = gpu._p

    def call(ix=h, n=3, rule=0, nq_=C.byref(nq), ids=P(q)):
        return lib.freddy_gpu_knn_join_ids(ix, None, ids, n, rule, 5, P(tg), 2, 1, 3, 0, 1, C.c_float(0.8), 10000000, P(oq), nq_, P(oi), P(od), C.byref(it))

    for kw, msg in ((dict(ix=None), "NULL index"), (dict(n=-1), "n_ids=-1"), (dict(rule=2), "bad id_rule 2"), (dict(rule=-1), "bad id_rule -1"),
                    (dict(nq_=None), "NULL n_queries"), (dict(ids=None), "NULL buffer")):
        assert call(**kw) == -1, kw                                                  # FREDDY_E_ARG
        assert msg in lib.freddy_gpu_last_error().decode(), (kw, lib.freddy_gpu_last_error())
    assert nq.value == -9 and it.value == -9 and (oq == -77).all() and (oi == -77).all() and (od == -77.0).all()
    # the analogy: its scalars first, then the handles
    t = np.array([[1, 2, 3]], np.int32)
    o1, o2 = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)

    def an(ix=h, v=h, Q=1, k=1, n_cand=4):
        return lib.freddy_gpu_ivpq_analogy(ix, v, P(t), Q, k, n_cand, P(tg), 2, 1, 3, 0, 1, C.c_float(0.8), 10000000, P(o1), P(o2))

    for kw, code, msg in ((dict(Q=-1), -1, "bad sizes"), (dict(k=0), -1, "bad sizes"), (dict(k=5), -1, "bad sizes"), (dict(n_cand=4097), -5, "n_cand = 4097"),
                          (dict(ix=None), -1, "NULL index"), (dict(v=None), -1, "NULL index"), (dict(ix=None, k=0), -1, "bad sizes")):
        assert an(**kw) == code, kw
        assert msg in lib.freddy_gpu_last_error().decode(), (kw, lib.freddy_gpu_last_error())


def test_the_host_mirror_has_them():
    h = open(os.path.join(ROOT, "include", "freddy_udf_ivpq.h")).read()
    for n in ("knn_in_ivpq_batch_ids", "analogy_3cosadd_in_ivpq_batch"):
        assert re.search(r"\b" + n + r"\(", h), n
    from freddy_amd import udf
    lib = udf.load()
    for n in ("knn_in_ivpq_batch_ids", "analogy_3cosadd_in_ivpq_batch"):
        assert hasattr(lib, n), n
    for m in ("knn_in_ivpq_batch_ids", "analogy_3cosadd_in_ivpq_batch"):
        assert callable(getattr(udf.Session, m, None)), m
