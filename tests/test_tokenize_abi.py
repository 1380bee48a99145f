"""Text vectors from token ids exist in every layer: the four entry points are exported by libfreddy_gpu.so, declared in
include/freddy_gpu.h (FREDDY_GPU_ABI_VERSION still 4: entry points only) and bound in freddy_amd/gpu.py; the host mirror exports
tokenize_batch and tokenize_raw_batch.  No GPU: the libraries are loaded and inspected, and the only calls made are refusals that
touch no device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("freddy_gpu_tokenize", "freddy_gpu_ivfadc_search_texts", "freddy_gpu_pq_search_texts", "freddy_gpu_exact_search_texts")
E_ARG = -1


def test_the_library_exports_them():
    from freddy_amd import gpu
    lib = gpu.load()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes, n
    assert lib.freddy_gpu_abi_version() == 4


def test_the_header_declares_them_and_keeps_its_abi_version():
    from freddy_amd import gpu
    lib = gpu.load()
    h = open(os.path.join(ROOT, "include", "freddy_gpu.h")).read()
    want = {
        "freddy_gpu_tokenize": ["vecs", "token_ids", "offsets", "n_texts", "id_rule", "normalize", "out_vectors", "out_count"],
        "freddy_gpu_ivfadc_search_texts": ["ivf", "vecs", "token_ids", "offsets", "n_texts", "id_rule", "k", "W", "sentinel", "found_rule",
                                           "out_count", "out_ids", "out_dist"],
        "freddy_gpu_pq_search_texts": ["pq", "vecs", "token_ids", "offsets", "n_texts", "id_rule", "k", "sentinel", "subset_ids", "n_subset",
                                       "out_count", "out_ids", "out_dist"],
        "freddy_gpu_exact_search_texts": ["vecs", "token_ids", "offsets", "n_texts", "id_rule", "normalize", "k", "subset_ids", "n_subset",
                                          "out_count", "out_ids", "out_sim"],
    }
    for n in NAMES:
        m = re.search(r"\bint " + n + r"\(([^;]*)\);", h)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1))
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == want[n], n
        assert len(getattr(lib, n).argtypes) == len(want[n]), n
    assert "#define FREDDY_GPU_ABI_VERSION 4" in h
    assert "#define FREDDY_TOK_MAX_LEN 4096" in h
    for opt in ('"tokenize_pass"', '"tokenize_unit"'):
        assert opt in h, opt


def test_the_binding_lists_and_wraps_them():
    from freddy_amd import gpu
    for n in NAMES:
        assert n in gpu.EXPORTS, n
    assert callable(getattr(gpu.VectorIndex, "tokenize", None))
    for cls in (gpu.VectorIndex, gpu.IVFIndex, gpu.PQIndex):
        assert callable(getattr(cls, "search_texts", None)), cls
    assert gpu.ABI_VERSION == 4 and gpu.TOK_MAX_LEN == 4096
    ids, off = gpu._texts([[3, 1], [], [7]])
    assert ids.dtype == np.int32 and off.dtype == np.int64 and ids.tolist() == [3, 1, 7] and off.tolist() == [0, 2, 2, 3]
    ids2, off2 = gpu._texts((np.array([3, 1, 7]), np.array([0, 2, 2, 3])))
    assert ids2.tolist() == ids.tolist() and off2.tolist() == off.tolist() and off2.dtype == np.int64


def test_the_host_mirror_exports_its_two_functions():
    from freddy_amd import udf
    lib = udf.load()
    for n in ("tokenize_batch", "tokenize_raw_batch"):
        assert hasattr(lib, n), n
        assert callable(getattr(udf.Session, n, None)), n
    h = open(os.path.join(ROOT, "include", "freddy_udf.h")).read()
    for n in ("tokenize_batch", "tokenize_raw_batch"):
        assert re.search(r"\bint " + n + r"\(freddy_session_t\* s, const int32_t\* token_ids, const int64_t\* offsets, int32_t n_texts,", h), n
    assert "stays with SQL;" not in h and "has a device form" in h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_refusals_that_touch_no_device():
    """a NULL handle, n_texts < 0, offsets that do not start at 0 or decrease, a bad rule: FREDDY_E_ARG, and the outputs untouched"""
    from freddy_amd import gpu
    lib = gpu.load()
    ids = np.array([1, 2, 3], np.int32)
    good, from_one, down = (np.array(o, np.int64) for o in ([0, 1, 3], [1, 2, 3], [0, 2, 1]))
    vec = np.full((2, 4), 7.0, np.float32)
    cnt = np.full(2, 7, np.int32)
    oi = np.full((2, 3), 7, np.int32)
    ov = np.full((2, 3), 7.0, np.float32)
    null = C.c_void_p()
    calls = {
        "tokenize": lambda off, n, rule=0: lib.freddy_gpu_tokenize(null, _p(ids), _p(off), n, rule, 1, _p(vec), _p(cnt)),
        "ivfadc": lambda off, n, rule=0: lib.freddy_gpu_ivfadc_search_texts(null, null, _p(ids), _p(off), n, rule, 3, 2, C.c_float(1000.0), 0,
                                                                             _p(cnt), _p(oi), _p(ov)),
        "pq": lambda off, n, rule=0: lib.freddy_gpu_pq_search_texts(null, null, _p(ids), _p(off), n, rule, 3, C.c_float(100.0), None, 0,
                                                                     _p(cnt), _p(oi), _p(ov)),
        "exact": lambda off, n, rule=0: lib.freddy_gpu_exact_search_texts(null, _p(ids), _p(off), n, rule, 1, 3, None, 0, _p(cnt), _p(oi), _p(ov)),
    }
    for name, call in calls.items():
        assert call(good, 2) == E_ARG and b"NULL index" in lib.freddy_gpu_last_error(), name
        assert call(good, -1) == E_ARG and b"n_texts" in lib.freddy_gpu_last_error(), name
        assert call(from_one, 2) == E_ARG and b"offsets[0]" in lib.freddy_gpu_last_error(), name
        assert call(down, 2) == E_ARG and b"decrease" in lib.freddy_gpu_last_error(), name
        assert call(good, 2, 2) == E_ARG and b"id_rule" in lib.freddy_gpu_last_error(), name
    assert np.all(vec == 7.0) and np.all(cnt == 7) and np.all(oi == 7) and np.all(ov == 7.0)
