"""ctypes binding of the C ABI in include/freddy_gpu.h (libfreddy_gpu.so).

The library is the product; this module only marshals numpy arrays / device pointers
into it.  There is NO CPU fallback: if the shared object is missing or a call fails the
error is raised.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("FREDDY_GPU_SO") or os.path.join(_PKG, "libfreddy_gpu.so")   # (FREDDY_GPU_SO: the tools' -DFREDDY_LAB build)

FOUND_ROWS = 0
FOUND_ACCEPTED = 1
FOUND_BATCH_UDF = 2   # ivfadc_batch_search itself (W == 1): accepted-rows rule + its argmin cell limit of 1000
METHOD_PQ, METHOD_EXACT, METHOD_PQ_PV = 0, 1, 2
QIDS_TABLE_ORDER = 0   # search_ids: "WHERE id IN (...)" -- ascending ids, duplicates collapse, ids without a row vanish
QIDS_POSITIONAL = 1    # slot j answers ids[j]; an id without a row keeps its slot and gets fillers
ANALOGY_METHODS = {"3cosadd": 0, "3cosmul": 1, "pair_direction": 2}   # include/freddy_gpu.h FREDDY_ANALOGY_*

EXPORTS = [
    "freddy_gpu_pin_pq", "freddy_gpu_pin_ivf", "freddy_gpu_pin_ivpq", "freddy_gpu_unpin",
    "freddy_gpu_pq_search", "freddy_gpu_ivfadc_search", "freddy_gpu_knn_join",
    "freddy_gpu_ivfadc_search_dev", "freddy_gpu_pq_search_dev", "freddy_gpu_last_error",
    "freddy_gpu_profile_enable", "freddy_gpu_profile_read", "freddy_gpu_index_bytes",
    "freddy_gpu_last_scanned_rows", "freddy_gpu_filter_bound_violations", "freddy_gpu_filter_bound_checked", "freddy_gpu_pin_vectors", "freddy_gpu_exact_search", "freddy_gpu_grouping_pq",
    "freddy_gpu_encode", "freddy_gpu_set_option", "freddy_gpu_last_track", "freddy_gpu_last_probed_cells", "freddy_gpu_coarse_bound_checked",
    "freddy_gpu_insert_quantize", "freddy_gpu_append_rows", "freddy_gpu_update_codebook", "freddy_gpu_kmeans",
    "freddy_gpu_host_alloc", "freddy_gpu_host_free", "freddy_gpu_pin_ivf_multi", "freddy_gpu_replica_count",
    "freddy_gpu_last_track_sized", "freddy_gpu_abi_version", "freddy_gpu_exact_analogy",
    "freddy_gpu_last_analogy_stats", "freddy_gpu_exact_join", "freddy_gpu_last_exact_join_stats",
    "freddy_gpu_ivfadc_search_pv", "freddy_gpu_pq_search_pv", "freddy_gpu_last_pv_stats",
    "freddy_gpu_ivfadc_analogy", "freddy_gpu_pq_analogy", "freddy_gpu_last_approx_analogy_stats",
    "freddy_gpu_exact_assign", "freddy_gpu_pq_assign", "freddy_gpu_remove_rows", "freddy_gpu_update_rows",
    "freddy_gpu_set_statistics", "freddy_gpu_get_statistics", "freddy_gpu_create_statistics",
    "freddy_gpu_debug_alloc_fail_nth", "freddy_gpu_debug_alloc_track", "freddy_gpu_debug_alloc_stats",
    "freddy_gpu_scan_elastic_stats",
    "freddy_gpu_ivfadc_search_ids", "freddy_gpu_pq_search_ids", "freddy_gpu_ivfadc_search_pv_ids", "freddy_gpu_pq_search_pv_ids",
    "freddy_gpu_similarity_pairs", "freddy_gpu_similarity_matrix", "freddy_gpu_similarity_join",
    "freddy_gpu_cluster",
    "freddy_gpu_exact_search_ids", "freddy_gpu_exact_join_ids", "freddy_gpu_debug_resolve_ids",
    "freddy_gpu_knn_join_ids", "freddy_gpu_ivpq_analogy",
    "freddy_gpu_tokenize", "freddy_gpu_ivfadc_search_texts", "freddy_gpu_pq_search_texts", "freddy_gpu_exact_search_texts",
]
TOK_MAX_LEN = 4096   # include/freddy_gpu.h FREDDY_TOK_MAX_LEN: ids per text
ABI_VERSION = 4   # include/freddy_gpu.h FREDDY_GPU_ABI_VERSION this binding was written against
STAT_PASS = 1 << 22   # a copy of csrc/join.hip STAT_PASS (change both together): ids per pass of freddy_gpu_create_statistics


class FreddyGpuError(RuntimeError):
    code = None   # the FREDDY_E_* value of the failed call, where there was one


class PQDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("m", C.c_int32), ("K", C.c_int32), ("N", C.c_int64),
                ("codebook", C.c_void_p), ("ids", C.c_void_p), ("codes", C.c_void_p)]


class IVFDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("m", C.c_int32), ("K", C.c_int32), ("C", C.c_int32),
                ("N", C.c_int64), ("coarse", C.c_void_p), ("codebook", C.c_void_p),
                ("list_off", C.c_void_p), ("ids", C.c_void_p), ("codes", C.c_void_p)]


class VecDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("N", C.c_int64), ("ids", C.c_void_p), ("vectors", C.c_void_p)]


class IVPQDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("m", C.c_int32), ("K", C.c_int32),
                ("coarse_positions", C.c_int32), ("coarse_codes", C.c_int32), ("N", C.c_int64),
                ("codebook", C.c_void_p), ("coarse", C.c_void_p), ("ids", C.c_void_p),
                ("coarse_id", C.c_void_p), ("codes", C.c_void_p), ("vectors", C.c_void_p),
                ("stats", C.c_void_p)]


_lib = None


def load(path=None, optional=()):
    """dlopen the library (once).  Raises if it has not been built.  path / optional: a tool that times a build of an earlier
    commit beside this one loads that library instead, which may lack the entry points named in `optional` (calling one fails)."""
    global _lib, LIB_PATH
    if _lib is not None:
        if path and os.path.abspath(path) != os.path.abspath(LIB_PATH):
            raise FreddyGpuError(f"{LIB_PATH} is already loaded: a process binds one library, {path} needs a process of its own")
        return _lib
    if path:
        LIB_PATH = path
    try:
        # torch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
        # runtimes in one process fight over the device, so when torch is around let its copy
        # be the one the dynamic loader binds first.  (A PostgreSQL backend has no torch and
        # simply uses /opt/rocm's runtime.)
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    if not os.path.exists(LIB_PATH):
        raise FreddyGpuError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    if lib.freddy_gpu_abi_version() != ABI_VERSION:
        raise FreddyGpuError(f"{LIB_PATH} has ABI version {lib.freddy_gpu_abi_version()}, this binding expects {ABI_VERSION}: rebuild")
    lib.freddy_gpu_last_track_sized.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.freddy_gpu_last_error.restype = C.c_char_p
    lib.freddy_gpu_index_bytes.restype = C.c_int64
    lib.freddy_gpu_index_bytes.argtypes = [C.c_void_p]
    lib.freddy_gpu_last_scanned_rows.restype = C.c_int64
    lib.freddy_gpu_last_scanned_rows.argtypes = [C.c_void_p]
    lib.freddy_gpu_filter_bound_violations.restype = C.c_int64
    lib.freddy_gpu_filter_bound_violations.argtypes = [C.c_void_p]
    lib.freddy_gpu_filter_bound_checked.restype = C.c_int64
    lib.freddy_gpu_filter_bound_checked.argtypes = [C.c_void_p]
    lib.freddy_gpu_coarse_bound_checked.restype = C.c_int64
    lib.freddy_gpu_coarse_bound_checked.argtypes = [C.c_void_p]
    if "freddy_gpu_scan_elastic_stats" not in optional:
        lib.freddy_gpu_scan_elastic_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.freddy_gpu_pin_pq.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.freddy_gpu_pin_ivf.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.freddy_gpu_pin_ivpq.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.freddy_gpu_pin_ivf_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.freddy_gpu_replica_count.argtypes = [C.c_void_p]
    lib.freddy_gpu_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    lib.freddy_gpu_host_free.argtypes = [C.c_void_p]
    lib.freddy_gpu_unpin.argtypes = [C.c_void_p]
    lib.freddy_gpu_pin_vectors.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.freddy_gpu_exact_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p]
    lib.freddy_gpu_exact_analogy.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_void_p]
    lib.freddy_gpu_last_analogy_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, types in (("freddy_gpu_exact_join", [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_last_exact_join_stats", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_ivfadc_search_pv", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                         C.c_int32, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_search_pv", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                     C.c_int64, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_last_pv_stats", [C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_ivfadc_analogy", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                       C.c_int32, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_analogy", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                   C.c_int64, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_last_approx_analogy_stats", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_exact_assign", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_assign", [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])):
        if name in optional and not hasattr(lib, name):
            continue
        getattr(lib, name).argtypes = types
    # searches by row id.  (A library built from an earlier commit, which the A/B helpers load through FREDDY_GPU_SO, lacks them:
    # every other call works, search_ids fails with the loader's "undefined symbol".)
    for name, types in (("freddy_gpu_ivfadc_search_ids", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_search_ids", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_ivfadc_search_pv_ids", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                             C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_search_pv_ids", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        # similarities by row id (the same holds for them)
                        ("freddy_gpu_similarity_pairs", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_similarity_matrix", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                          C.c_void_p]),
                        ("freddy_gpu_similarity_join", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_int64,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                        # the whole k-means of cluster_exact / cluster_pq (the same again)
                        ("freddy_gpu_cluster", [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
                        # exact kNN / the exact join by row id, and the device resolve's test hook (the same again)
                        ("freddy_gpu_exact_search_ids", [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_exact_join_ids", [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_debug_resolve_ids", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                        # the kNN-join by row id and the batched analogy over it (the same again)
                        ("freddy_gpu_knn_join_ids", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_ivpq_analogy", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
                        # text vectors from token ids and the searches over them (the same again)
                        ("freddy_gpu_tokenize", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_ivfadc_search_texts", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                            C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_pq_search_texts", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
                        ("freddy_gpu_exact_search_texts", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = types
    lib.freddy_gpu_pq_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_ivfadc_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_knn_join.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_ivfadc_search_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    lib.freddy_gpu_pq_search_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_last_probed_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_insert_quantize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
    lib.freddy_gpu_append_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_update_codebook.argtypes = [C.c_void_p, C.c_void_p]
    if "freddy_gpu_remove_rows" not in optional:
        lib.freddy_gpu_remove_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    if "freddy_gpu_update_rows" not in optional:
        lib.freddy_gpu_update_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, types in (("freddy_gpu_set_statistics", [C.c_void_p, C.c_void_p, C.c_int32]),
                        ("freddy_gpu_get_statistics", [C.c_void_p, C.c_void_p, C.c_int32]),
                        ("freddy_gpu_create_statistics", [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p])):
        if name not in optional:
            getattr(lib, name).argtypes = types
    lib.freddy_gpu_kmeans.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.freddy_gpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.freddy_gpu_last_track.argtypes = [C.c_void_p, C.c_void_p]
    lib.freddy_gpu_profile_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.freddy_gpu_profile_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, types in (("freddy_gpu_debug_alloc_fail_nth", [C.c_int64, C.c_int32]), ("freddy_gpu_debug_alloc_track", [C.c_int32]),
                        ("freddy_gpu_debug_alloc_stats", [C.c_void_p, C.c_size_t])):
        if name not in optional:
            getattr(lib, name).argtypes = types
    _lib = lib
    return lib


E_NOMEM = -3   # include/freddy_gpu.h FREDDY_E_NOMEM


class AllocStats(C.Structure):
    """freddy_alloc_stats (include/freddy_gpu.h)"""
    _fields_ = [("calls", C.c_int64), ("failed", C.c_int64), ("live", C.c_int64), ("live_bytes", C.c_int64), ("digest", C.c_uint64)]


def alloc_fail_nth(n, real=False):
    """The n-th device / pinned-host allocation from now fails once (freddy_gpu_debug_alloc_fail_nth); n <= 0 disarms."""
    _check(load().freddy_gpu_debug_alloc_fail_nth(int(n), 1 if real else 0))


def alloc_track(on):
    """Track the live allocations from an empty set (freddy_gpu_debug_alloc_track)."""
    _check(load().freddy_gpu_debug_alloc_track(1 if on else 0))


def alloc_stats():
    """-> AllocStats: calls, failed, live, live_bytes, digest (freddy_gpu_debug_alloc_stats)."""
    st = AllocStats()
    n = load().freddy_gpu_debug_alloc_stats(C.byref(st), C.sizeof(st))
    if n != C.sizeof(st):
        raise FreddyGpuError(f"freddy_gpu_debug_alloc_stats wrote {n} of {C.sizeof(st)} bytes")
    return st


def _check(rc):
    if rc != 0:
        err = FreddyGpuError(f"freddy_gpu error {rc}: {load().freddy_gpu_last_error().decode()}")
        err.code = rc   # (the FREDDY_E_* value, for callers that tell a failed allocation from the rest)
        raise err


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i16(a):
    return np.ascontiguousarray(a, dtype=np.int16)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Index:
    kind = "?"

    def __init__(self):
        self.h = C.c_void_p()
        self.lib = load()

    def close(self):
        if self.h:
            self.lib.freddy_gpu_unpin(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def nbytes(self):
        return int(self.lib.freddy_gpu_index_bytes(self.h))

    def append_rows(self, ids, coarse_id=None, codes=None, vectors=None):
        """INSERT of new rows into the pinned tables (freddy_gpu_append_rows): ids ascending beyond the pinned ones."""
        ids = _i32(ids)
        cid = None if coarse_id is None else _i32(coarse_id)
        cd = None if codes is None else _i16(codes)
        v = None if vectors is None else _f32(vectors)
        _check(self.lib.freddy_gpu_append_rows(self.h, ids.size, _p(ids), _p(cid), _p(cd), _p(v)))
        self.N += ids.size   # (grouping() sizes its output arrays by it)

    def remove_rows(self, ids):
        """DELETE of rows from the pinned tables (freddy_gpu_remove_rows): ids in any order, unknown ids are skipped, an id listed
        twice counts once.  -> the number of rows that left."""
        ids = np.asarray(ids)
        if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise FreddyGpuError("row ids are 32-bit integers")
        ids = _i32(ids).reshape(-1)
        gone = C.c_int64(0)
        _check(self.lib.freddy_gpu_remove_rows(self.h, ids.size, _p(ids), C.byref(gone)))
        self.N -= gone.value   # (grouping() sizes its output arrays by it)
        return int(gone.value)

    def update_rows(self, ids, coarse_id=None, codes=None, vectors=None):
        """UPDATE of rows of the pinned tables (freddy_gpu_update_rows): every pinned row whose id is ids[i] gets the i-th payload
        (the arrays append_rows takes for the handle's kind) and keeps its id.  ids in any order, unknown ids are skipped, an id
        listed twice is refused.  -> the number of rows that changed."""
        ids = np.asarray(ids)
        if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise FreddyGpuError("row ids are 32-bit integers")
        ids = _i32(ids).reshape(-1)
        cid = None if coarse_id is None else _i32(coarse_id)
        cd = None if codes is None else _i16(codes)
        v = None if vectors is None else _f32(vectors)
        # the library reads ids.size rows of each array it is given: m codes, d floats (a borrowed handle knows neither: the caller's part)
        for name, a, per_row in (("coarse_id", cid, 1), ("codes", cd, getattr(self, "m", None)), ("vectors", v, getattr(self, "d", None))):
            if a is not None and per_row is not None and a.size != ids.size * per_row:
                raise FreddyGpuError(f"{name} has {a.size} elements, {ids.size} ids need {ids.size * per_row}")
        changed = C.c_int64(0)
        _check(self.lib.freddy_gpu_update_rows(self.h, ids.size, _p(ids), _p(cid), _p(cd), _p(v), C.byref(changed)))
        return int(changed.value)

    def update_codebook(self, codebook):
        cb = _f32(codebook)
        _check(self.lib.freddy_gpu_update_codebook(self.h, _p(cb)))

    def bound_violations(self):
        """Rows of the filter + refine scan's exact stage whose distance left the proven bracket (must be 0)."""
        return int(self.lib.freddy_gpu_filter_bound_violations(self.h))

    def scan_elastic_stats(self):
        """The elastic scan's device words (freddy_gpu_scan_elastic_stats; synchronises the device): scan workgroups alive and
        announced (both 0 between searches), extras that took work and extras that left for another scan since the pin."""
        v = (C.c_int64 * 4)()
        _check(self.lib.freddy_gpu_scan_elastic_stats(self.h, v))
        return {"active": int(v[0]), "pending": int(v[1]), "started": int(v[2]), "yielded": int(v[3])}

    def set_option(self, name, value):
        """Tuning / debug switch of this pinned index (include/freddy_gpu.h: freddy_gpu_set_option)."""
        _check(self.lib.freddy_gpu_set_option(self.h, name.encode(), int(value)))

    def profile_enable(self, on=True):
        _check(self.lib.freddy_gpu_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        cap = 32
        names = ((C.c_char * 64) * cap)()
        launches = (C.c_int64 * cap)()
        ms = (C.c_double * cap)()
        n = self.lib.freddy_gpu_profile_read(self.h, cap, names, launches, ms)
        if n < 0:
            _check(n)
        return {names[i].value.decode(): (int(launches[i]), float(ms[i])) for i in range(min(n, cap))}

    def last_pv_stats(self):
        """The last search_pv() call on this pq / ivf handle (freddy_gpu_last_pv_stats): list entries with id >= 0 summed over the
        queries, and how many of them had a vector row."""
        v = [C.c_int64(0) for _ in range(2)]
        _check(self.lib.freddy_gpu_last_pv_stats(self.h, *(C.byref(x) for x in v)))
        return {"candidates": v[0].value, "scored": v[1].value}

    def last_approx_analogy_stats(self):
        """The last analogy() call on this pq / ivf / ivpq handle (freddy_gpu_last_approx_analogy_stats): triples that reached stage one,
        their list entries with id >= 0, and how many of those had a vector row and were not an input of their triple."""
        v = [C.c_int64(0) for _ in range(3)]
        _check(self.lib.freddy_gpu_last_approx_analogy_stats(self.h, *(C.byref(x) for x in v)))
        return {"searched": v[0].value, "candidates": v[1].value, "scored": v[2].value}


def _search_ids(ids, k, call):
    """The buffers of a search by row id: call(query_ids, n_ids, out_query_ids, n_queries, out_ids, out_values) -> the outputs cut to
    n_queries."""
    q = _i32(ids).reshape(-1)
    n = q.size
    rows = max(n, 1) * max(int(k), 1)
    out_q = np.empty(max(n, 1), np.int32)
    out_i = np.empty(rows, np.int32)
    out_v = np.empty(rows, np.float32)
    nq = C.c_int32(-1)
    _check(call(q, n, out_q, nq, out_i, out_v))
    Q = nq.value
    return out_q[:Q], out_i[:Q * k].reshape(Q, k), out_v[:Q * k].reshape(Q, k)


def _texts(texts):
    """The texts of a tokenize / search_texts call as (token_ids int32, offsets int64[n + 1]): a sequence of id sequences, or an
    (ids, offsets) pair -- a TUPLE whose second member is a numpy array, the offsets."""
    if isinstance(texts, tuple) and len(texts) == 2 and isinstance(texts[1], np.ndarray):
        ids, off = _i32(texts[0]).reshape(-1), np.ascontiguousarray(texts[1], dtype=np.int64).reshape(-1)
        if off.size < 1:
            raise FreddyGpuError("offsets needs n_texts + 1 entries")
        return ids, off
    lens = [len(t) for t in texts]
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.concatenate([_i32(t).reshape(-1) for t in texts]) if lens else np.empty(0, np.int32)
    return _i32(ids), off


def _search_texts(texts, k, call):
    """The buffers of a search over texts: call(token_ids, offsets, n_texts, out_count, out_ids, out_values) -> (counts[n], ids[n,k],
    values[n,k])."""
    ids, off = _texts(texts)
    n = off.size - 1
    cnt = np.empty(max(n, 1), np.int32)
    out_i = np.empty((max(n, 1), k), np.int32)
    out_v = np.empty((max(n, 1), k), np.float32)
    _check(call(ids, off, n, cnt, out_i, out_v))
    return cnt[:n], out_i[:n], out_v[:n]


class PQIndex(_Index):
    """pq_codebook + pq_quantization pinned in HBM."""
    kind = "pq"

    def __init__(self, codebook, ids, codes, device=0):
        super().__init__()
        cb, ids, codes = _f32(codebook), _i32(ids), _i16(codes)
        m, K, s = cb.shape
        assert codes.shape == (ids.size, m)
        self.d, self.m, self.K, self.N = m * s, m, K, ids.size
        desc = PQDesc(self.d, m, K, ids.size, _p(cb), _p(ids), _p(codes))
        _check(self.lib.freddy_gpu_pin_pq(C.byref(desc), device, C.byref(self.h)))

    def search(self, queries, k, sentinel=100.0, subset_ids=None):
        """(ids[Q,k], dist[Q,k]); subset_ids=None -> pq_search, else pq_search_in[_batch]."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_d = np.empty((Q, k), np.float32)
        sub = None if subset_ids is None else _i32(subset_ids)
        _check(self.lib.freddy_gpu_pq_search(self.h, _p(qs), Q, k, C.c_float(sentinel), _p(sub),
                                             0 if sub is None else sub.size, _p(out_i), _p(out_d)))
        return out_i, out_d

    def search_pv(self, vecs, queries, k, pvf, sentinel=100.0, subset_ids=None):
        """pq_search at k * pvf, re-ranked on the device against the VectorIndex `vecs` (freddy_gpu_pq_search_pv):
        (ids[Q,k], similarity[Q,k]), bit for bit vecs.search(q, k, subset_ids=<the candidates of q>) per query."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        sub = None if subset_ids is None else _i32(subset_ids)
        _check(self.lib.freddy_gpu_pq_search_pv(self.h, vecs.h, _p(qs), Q, k, pvf, C.c_float(sentinel), _p(sub),
                                                0 if sub is None else sub.size, _p(out_i), _p(out_s)))
        return out_i, out_s

    def search_ids(self, vecs, ids, k, sentinel=100.0, subset_ids=None, rule=QIDS_TABLE_ORDER):
        """pq_search for the rows of the VectorIndex `vecs` with these ids, gathered on the device (freddy_gpu_pq_search_ids):
        (query_ids[Q], ids[Q,k], dist[Q,k]) with Q = the queries `rule` selects; per query bit for bit search(<its row of vecs>, k, ...)."""
        sub = None if subset_ids is None else _i32(subset_ids)
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_pq_search_ids(
            self.h, vecs.h, _p(q), n, rule, k, C.c_float(sentinel), _p(sub), 0 if sub is None else sub.size, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def search_texts(self, vecs, texts, k, sentinel=100.0, subset_ids=None, rule=QIDS_TABLE_ORDER):
        """pq_search for the text vectors vecs.tokenize(texts) computes, which stay on the device (freddy_gpu_pq_search_texts):
        (counts[n], ids[n,k], dist[n,k]); per text with a row list bit for bit search(<its vector>, k, ...), fillers for the others."""
        sub = None if subset_ids is None else _i32(subset_ids)
        return _search_texts(texts, k, lambda t, o, n, oc, oi, od: self.lib.freddy_gpu_pq_search_texts(
            self.h, vecs.h, _p(t), _p(o), n, rule, k, C.c_float(sentinel), _p(sub), 0 if sub is None else sub.size, _p(oc), _p(oi), _p(od)))

    def search_pv_ids(self, vecs, ids, k, pvf, sentinel=100.0, subset_ids=None, rule=QIDS_TABLE_ORDER):
        """search_pv for the rows of `vecs` with these ids (freddy_gpu_pq_search_pv_ids): (query_ids[Q], ids[Q,k], similarity[Q,k])."""
        sub = None if subset_ids is None else _i32(subset_ids)
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_pq_search_pv_ids(
            self.h, vecs.h, _p(q), n, rule, k, pvf, C.c_float(sentinel), _p(sub), 0 if sub is None else sub.size, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def analogy(self, vecs, triples, k=1, n_cand=23, sentinel=100.0, subset_ids=None):
        """Approximate 3CosAdd analogies (freddy_gpu_pq_analogy): triples [Q][3] of row ids (w1, w2, w3) -> (ids[Q,k], similarity[Q,k]);
        per triple bit for bit vecs.search(v3 - v1 + v2, k, subset_ids=<the n_cand candidates of pq_search for the normalised sum,
        without the inputs>); (-1, -inf) where there is no row or an input id has no vector.  subset_ids: analogy_3cosadd_in_pq."""
        t = _i32(triples).reshape(-1, 3)
        Q = t.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        sub = None if subset_ids is None else _i32(subset_ids)
        _check(self.lib.freddy_gpu_pq_analogy(self.h, vecs.h, _p(t), Q, k, n_cand, C.c_float(sentinel), _p(sub),
                                              0 if sub is None else sub.size, _p(out_i), _p(out_s)))
        return out_i, out_s

    def bind_search(self, queries, k, sentinel=100.0):
        """pq_search through the host-buffer call with every argument converted ONCE (the caller's loop then costs what a C
        caller's costs): returns (call, out_ids, out_dist); call() fills the two arrays."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_d = np.empty((Q, k), np.float32)
        fn = self.lib.freddy_gpu_pq_search
        args = (self.h, _p(qs), C.c_int32(Q), C.c_int32(k), C.c_float(sentinel), None, C.c_int64(0), _p(out_i), _p(out_d))

        def call(_keep=(qs,)):
            rc = fn(*args)
            if rc != 0:
                _check(rc)
        return call, out_i, out_d

    def grouping(self, group_vectors, subset_ids=None):
        """grouping_pq: (ids, group index) of every (requested) row; groups tried in the given order."""
        gv = _f32(group_vectors).reshape(-1, self.d)
        sub = None if subset_ids is None else _i32(subset_ids)
        cap = self.N if sub is None else max(sub.size, 1)
        oi = np.empty(cap, np.int32); og = np.empty(cap, np.int32)
        n = C.c_int64(0)
        _check(self.lib.freddy_gpu_grouping_pq(self.h, _p(gv), gv.shape[0], _p(sub), 0 if sub is None else sub.size,
                                               _p(oi), _p(og), C.byref(n)))
        return oi[:n.value], og[:n.value]

    def assign(self, queries, target_ids, sentinel=1000.0):
        """The assignment step of cluster_pq (freddy_gpu_pq_assign): (query index[n], similarity[n]), slot i for target_ids[i] -- the
        first query under "freddy_similarity_of(ADC distance) DESC, query index ASC" among those with distance < sentinel;
        (-1, -inf) where there is none or the id has no row."""
        return _assign(self, self.lib.freddy_gpu_pq_assign, queries, target_ids, (C.c_float(sentinel),))

    def search_dev(self, d_queries_ptr, Q, k, sentinel, d_out_ids_ptr, d_out_dist_ptr, stream=None):
        _check(self.lib.freddy_gpu_pq_search_dev(self.h, C.c_void_p(d_queries_ptr), Q, k, C.c_float(sentinel),
                                                 C.c_void_p(d_out_ids_ptr), C.c_void_p(d_out_dist_ptr),
                                                 C.c_void_p(stream or 0)))


def _assign(ix, fn, queries, target_ids, extra, d=None):
    """The two assign entry points on a handle object (ix.h; d: the table's dimension where the object does not know it)."""
    qs = _f32(queries).reshape(-1, d or ix.d)
    t = _i32(target_ids).reshape(-1)
    out_q = np.empty(t.size, np.int32)
    out_s = np.empty(t.size, np.float32)
    _check(fn(ix.h, _p(qs) if qs.size else None, qs.shape[0], *extra, _p(t) if t.size else None, t.size, _p(out_q), _p(out_s)))
    return out_q, out_s


class VectorIndex(_Index):
    """google_vecs_norm pinned as raw vectors: exact brute-force kNN."""
    kind = "vec"

    def __init__(self, ids, vectors, device=0):
        super().__init__()
        ids, v = _i32(ids), _f32(vectors)
        self.d, self.N = v.shape[1], ids.size
        desc = VecDesc(self.d, ids.size, _p(ids), _p(v))
        _check(self.lib.freddy_gpu_pin_vectors(C.byref(desc), device, C.byref(self.h)))

    def search(self, queries, k, subset_ids=None):
        """(ids[Q,k], similarity[Q,k]) ORDER BY cosine_similarity_bytea DESC, id ASC."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        sub = None if subset_ids is None else _i32(subset_ids)
        _check(self.lib.freddy_gpu_exact_search(self.h, _p(qs), Q, k, _p(sub), 0 if sub is None else sub.size,
                                                _p(out_i), _p(out_s)))
        return out_i, out_s

    def analogy(self, triples, k=1, method="3cosmul", subset_ids=None):
        """Exact analogies (freddy_gpu_exact_analogy): triples [Q][3] of row ids (w1, w2, w3) -> (ids[Q,k], scores[Q,k] float64),
        ORDER BY score DESC, id ASC, the three inputs excluded; (-1, -inf) where there is no row (or an input id is unknown).
        method: "3cosadd" (the binary32 score widened), "3cosmul" (float8) or "pair_direction" (analogy_pair_direction: binary32
        widened; meant for a handle that holds the original, un-normalised table)."""
        if method not in ANALOGY_METHODS:
            raise ValueError(f"method must be one of {sorted(ANALOGY_METHODS)}")
        t = _i32(triples).reshape(-1, 3)
        Q = t.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float64)
        sub = None if subset_ids is None else _i32(subset_ids)
        _check(self.lib.freddy_gpu_exact_analogy(self.h, ANALOGY_METHODS[method], _p(t), Q, k, _p(sub), 0 if sub is None else sub.size,
                                                 _p(out_i), _p(out_s)))
        return out_i, out_s

    def last_analogy_stats(self):
        """The last analogy() call (freddy_gpu_last_analogy_stats): filter passes, candidates they refined, passes redone all-exact."""
        v = [C.c_int64(0) for _ in range(3)]
        _check(self.lib.freddy_gpu_last_analogy_stats(self.h, *(C.byref(x) for x in v)))
        return {"filter_passes": v[0].value, "candidates": v[1].value, "redone_passes": v[2].value}

    def join(self, queries, k, target_ids):
        """The exact kNN-join (freddy_gpu_exact_join): (ids[Q,k], similarity[Q,k]) of every query over the rows whose id is in
        target_ids -- bit for bit search(queries, k, subset_ids=target_ids); an empty target_ids is the empty set."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        t = _i32(target_ids).reshape(-1)
        _check(self.lib.freddy_gpu_exact_join(self.h, _p(qs), Q, k, _p(t) if t.size else None, t.size, _p(out_i), _p(out_s)))
        return out_i, out_s

    def exact_search_ids(self, ids, k, subset_ids=None, rule=QIDS_TABLE_ORDER):
        """search() for the rows of this table with these ids (freddy_gpu_exact_search_ids): (query_ids[Q], ids[Q,k], similarity[Q,k])
        with Q = the queries `rule` selects; per query bit for bit search(<its row>, k, subset_ids).  The subset is resolved on the device."""
        sub = None if subset_ids is None else _i32(subset_ids).reshape(-1)
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_exact_search_ids(
            self.h, _p(q), n, rule, k, _p(sub), 0 if sub is None else sub.size, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def tokenize(self, texts, normalize=True, rule=QIDS_TABLE_ORDER):
        """Text vectors from token ids (freddy_gpu_tokenize; tokenize() / tokenize_raw() of the SQL surface): texts is a sequence of
        sequences of row ids of this table, or an (ids, offsets) pair -> (vectors[n,d], counts[n]).  The vector of a text is the
        reference's centroid of its rows (rule: the distinct rows in table order, or the given rows in the given order), normalised
        unless normalize is false; a text without a row has count 0 and a vector of zeros."""
        ids, off = _texts(texts)
        n = off.size - 1
        out = np.empty((max(n, 1), self.d), np.float32)
        cnt = np.empty(max(n, 1), np.int32)
        _check(self.lib.freddy_gpu_tokenize(self.h, _p(ids), _p(off), n, rule, 1 if normalize else 0, _p(out), _p(cnt)))
        return out[:n], cnt[:n]

    def search_texts(self, texts, k, normalize=True, subset_ids=None, rule=QIDS_TABLE_ORDER):
        """search() for the text vectors tokenize(texts, normalize, rule) computes, which stay on the device
        (freddy_gpu_exact_search_texts): (counts[n], ids[n,k], similarity[n,k]); (-1, -inf) for a text without a row."""
        sub = None if subset_ids is None else _i32(subset_ids).reshape(-1)
        return _search_texts(texts, k, lambda t, o, n, oc, oi, od: self.lib.freddy_gpu_exact_search_texts(
            self.h, _p(t), _p(o), n, rule, 1 if normalize else 0, k, _p(sub), 0 if sub is None else sub.size, _p(oc), _p(oi), _p(od)))

    def exact_join_ids(self, ids, k, target_ids, rule=QIDS_TABLE_ORDER):
        """join() for the rows of this table with these ids (freddy_gpu_exact_join_ids): (query_ids[Q], ids[Q,k], similarity[Q,k]); per
        query bit for bit join(<its row>, k, target_ids).  The target set is resolved on the device; an empty one is the empty set."""
        t = _i32(target_ids).reshape(-1)
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_exact_join_ids(
            self.h, _p(q), n, rule, k, _p(t) if t.size else None, t.size, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def debug_resolve_ids(self, ids):
        """The device resolve alone (freddy_gpu_debug_resolve_ids): the table rows of `ids`, ascending and distinct."""
        t = _i32(ids).reshape(-1)
        out = np.empty(max(t.size, 1), np.int32)   # (min(n, N) entries are written at most)
        n = C.c_int64(-1)
        _check(self.lib.freddy_gpu_debug_resolve_ids(self.h, _p(t) if t.size else None, t.size, _p(out), C.byref(n)))
        return out[:n.value].copy()

    def assign(self, queries, target_ids):
        """The assignment step of cluster_exact (freddy_gpu_exact_assign): (query index[n], similarity[n]), slot i for
        target_ids[i] -- the first query under "cosine_similarity_bytea DESC (PostgreSQL's float4 order), query index ASC", the
        similarity bits of join(); (-1, -inf) where the id has no row."""
        return _assign(self, self.lib.freddy_gpu_exact_assign, queries, target_ids, ())

    def cluster(self, token_ids, kc, draws, rounds=10, pq=None, sentinel=1000.0):
        """The whole k-means of cluster_exact (pq=None) / cluster_pq (pq: a PQIndex) in one call (freddy_gpu_cluster): (clusters[n] int32,
        1 .. kc or 0 for a position no round claimed; similarity[n] of the last round, -inf where it claimed nothing; centroids[kc, d]
        the last assignment used).  draws: the float64 values of random(), kc + 10 * kc * (rounds - 1) of them at least."""
        t = _i32(token_ids).reshape(-1)
        dr = np.ascontiguousarray(draws, np.float64).reshape(-1)
        kc = int(kc)
        out_c = np.empty(t.size, np.int32)
        out_s = np.empty(t.size, np.float32)
        out_m = np.empty((max(kc, 0), self.d), np.float32)
        _check(self.lib.freddy_gpu_cluster(self.h, None if pq is None else pq.h, C.c_float(sentinel), _p(t) if t.size else None, t.size, kc, int(rounds),
                                           _p(dr) if dr.size else None, dr.size, _p(out_c), _p(out_s), _p(out_m)))
        return out_c, out_s, out_m

    def similarity_pairs(self, ids_a, ids_b):
        """cosine_similarity(token1, token2) for n pairs of row ids (freddy_gpu_similarity_pairs): (sim[n] float32, known[n] bool);
        a pair with an id that has no row is (0.0, False)."""
        a, b = _i32(ids_a).reshape(-1), _i32(ids_b).reshape(-1)
        if a.size != b.size:
            raise FreddyGpuError(f"ids_a has {a.size} ids, ids_b {b.size}")
        sim = np.empty(a.size, np.float32)
        known = np.empty(a.size, np.uint8)
        _check(self.lib.freddy_gpu_similarity_pairs(self.h, _p(a), _p(b), a.size, _p(sim), _p(known)))
        return sim, known.astype(bool)

    def _sim_a(self, a):
        """The A side of similarity_matrix / similarity_join: an integer array is row ids, a 2-d float array is vectors -> (ids, vectors, na)"""
        a = np.asarray(a)
        if np.issubdtype(a.dtype, np.integer):
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise FreddyGpuError("row ids are 32-bit integers")
            ids = _i32(a).reshape(-1)
            return ids, None, ids.size
        if a.ndim != 2 or a.shape[1] != self.d or not np.issubdtype(a.dtype, np.floating):
            raise FreddyGpuError(f"the A side is an integer array of row ids or a float array [na][{self.d}]")
        v = _f32(a)
        return None, v, v.shape[0]

    def similarity_matrix(self, a, b_ids):
        """All similarities of A (row ids, or [na][d] float vectors: cosine_similarity_bytea(vector, token)) against the rows of b_ids
        (freddy_gpu_similarity_matrix): (out[na, nb] float32, known_a[na] bool, known_b[nb] bool); entries of an id without a row are 0.0."""
        ids, v, na = self._sim_a(a)
        b = _i32(b_ids).reshape(-1)
        out = np.empty((na, b.size), np.float32)
        ka, kb = np.empty(na, np.uint8), np.empty(b.size, np.uint8)
        # (a side without elements still names itself: the library refuses "both or neither")
        _check(self.lib.freddy_gpu_similarity_matrix(self.h, _p(ids) if ids is not None else None, _p(v) if v is not None else None, na,
                                                     _p(b), b.size, _p(out), _p(ka), _p(kb)))
        return out, ka.astype(bool), kb.astype(bool)

    def similarity_join(self, a, b_ids, threshold, max_pairs=None):
        """WHERE cosine_similarity(a, b) > threshold (freddy_gpu_similarity_join; PostgreSQL's float4 order): (ia, ib, sim, total) --
        0-based positions in a and b_ids and the value of the first min(total, max_pairs) matches, i ascending then j ascending; total
        counts every match.  max_pairs=None: a count call first, then all of them."""
        ids, v, na = self._sim_a(a)
        b = _i32(b_ids).reshape(-1)
        total = C.c_int64(0)

        def call(cap, ia, ib, sim):
            _check(self.lib.freddy_gpu_similarity_join(self.h, _p(ids) if ids is not None else None, _p(v) if v is not None else None, na,
                                                       _p(b), b.size, C.c_float(threshold), cap, _p(ia), _p(ib), _p(sim), C.byref(total)))
        counted = max_pairs is None
        if counted:
            call(0, None, None, None)
            max_pairs = total.value
        max_pairs = int(max_pairs)
        ia, ib, sim = np.empty(max_pairs, np.int32), np.empty(max_pairs, np.int32), np.empty(max_pairs, np.float32)
        if max_pairs > 0 or not counted:
            call(max_pairs, ia, ib, sim)
        n = min(int(total.value), int(max_pairs))
        return ia[:n], ib[:n], sim[:n], int(total.value)

    def last_join_stats(self):
        """The last join() call (freddy_gpu_last_exact_join_stats): queries the filter ran for, candidates refined, queries redone all-exact."""
        v = [C.c_int64(0) for _ in range(3)]
        _check(self.lib.freddy_gpu_last_exact_join_stats(self.h, *(C.byref(x) for x in v)))
        return {"filter_queries": v[0].value, "candidates": v[1].value, "redone_queries": v[2].value}

    def bound_checked(self):
        """Rows the self-check has compared with their bracket (option check_brackets bits 2 / 3 refine every row)."""
        return int(self.lib.freddy_gpu_filter_bound_checked(self.h))


class IVFIndex(_Index):
    """coarse_quantization + residual_codebook + fine_quantization pinned in HBM."""
    kind = "ivf"

    def __init__(self, coarse, codebook, list_off, ids, codes, device=0, devices=None):
        """devices: a list of device ordinals -> the tables replicated on each of them behind one handle
        (freddy_gpu_pin_ivf_multi); host batches are then split contiguously over the devices."""
        super().__init__()
        cq, cb, lo, ids, codes = _f32(coarse), _f32(codebook), _i32(list_off), _i32(ids), _i16(codes)
        m, K, s = cb.shape
        assert cq.shape[1] == m * s and lo.size == cq.shape[0] + 1
        self.d, self.m, self.K, self.C, self.N = m * s, m, K, cq.shape[0], ids.size
        desc = IVFDesc(self.d, m, K, self.C, ids.size, _p(cq), _p(cb), _p(lo), _p(ids), _p(codes))
        if devices is None:
            _check(self.lib.freddy_gpu_pin_ivf(C.byref(desc), device, C.byref(self.h)))
        else:
            devs = (C.c_int * len(devices))(*devices)
            _check(self.lib.freddy_gpu_pin_ivf_multi(C.byref(desc), devs, len(devices), C.byref(self.h)))

    @property
    def replicas(self):
        return int(self.lib.freddy_gpu_replica_count(self.h))

    def search(self, queries, k, W, sentinel=1000.0, found_rule=FOUND_ROWS):
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_d = np.empty((Q, k), np.float32)
        _check(self.lib.freddy_gpu_ivfadc_search(self.h, _p(qs), Q, k, W, C.c_float(sentinel), found_rule,
                                                 _p(out_i), _p(out_d)))
        return out_i, out_d

    def search_pv(self, vecs, queries, k, pvf, W, sentinel=1000.0, found_rule=FOUND_ROWS):
        """ivfadc_search at k * pvf, re-ranked on the device against the VectorIndex `vecs` (freddy_gpu_ivfadc_search_pv):
        (ids[Q,k], similarity[Q,k]), bit for bit vecs.search(q, k, subset_ids=<the candidates of q>) per query."""
        qs = _f32(queries).reshape(-1, self.d)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        _check(self.lib.freddy_gpu_ivfadc_search_pv(self.h, vecs.h, _p(qs), Q, k, pvf, W, C.c_float(sentinel), found_rule,
                                                    _p(out_i), _p(out_s)))
        return out_i, out_s

    def search_texts(self, vecs, texts, k, W, sentinel=1000.0, found_rule=FOUND_ROWS, rule=QIDS_TABLE_ORDER):
        """ivfadc_search for the text vectors vecs.tokenize(texts) computes, which stay on the device (freddy_gpu_ivfadc_search_texts):
        (counts[n], ids[n,k], dist[n,k]); per text with a row list bit for bit search(<its vector>, k, W, ...), fillers for the others."""
        return _search_texts(texts, k, lambda t, o, n, oc, oi, od: self.lib.freddy_gpu_ivfadc_search_texts(
            self.h, vecs.h, _p(t), _p(o), n, rule, k, W, C.c_float(sentinel), found_rule, _p(oc), _p(oi), _p(od)))

    def search_ids(self, vecs, ids, k, W, sentinel=1000.0, found_rule=FOUND_ROWS, rule=QIDS_TABLE_ORDER):
        """ivfadc_search for the rows of the VectorIndex `vecs` with these ids, gathered on the device (freddy_gpu_ivfadc_search_ids):
        (query_ids[Q], ids[Q,k], dist[Q,k]) with Q = the queries `rule` selects; per query bit for bit search(<its row of vecs>, k, W, ...)."""
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_ivfadc_search_ids(
            self.h, vecs.h, _p(q), n, rule, k, W, C.c_float(sentinel), found_rule, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def search_pv_ids(self, vecs, ids, k, pvf, W, sentinel=1000.0, found_rule=FOUND_ROWS, rule=QIDS_TABLE_ORDER):
        """search_pv for the rows of `vecs` with these ids (freddy_gpu_ivfadc_search_pv_ids): (query_ids[Q], ids[Q,k], similarity[Q,k])."""
        return _search_ids(ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_ivfadc_search_pv_ids(
            self.h, vecs.h, _p(q), n, rule, k, pvf, W, C.c_float(sentinel), found_rule, _p(oq), C.byref(nq), _p(oi), _p(od)))

    def analogy(self, vecs, triples, k=1, n_cand=23, W=3, sentinel=1000.0, found_rule=FOUND_ROWS):
        """Approximate 3CosAdd analogies (freddy_gpu_ivfadc_analogy): triples [Q][3] of row ids (w1, w2, w3) -> (ids[Q,k],
        similarity[Q,k]); per triple bit for bit vecs.search(v3 - v1 + v2, k, subset_ids=<the n_cand candidates of ivfadc_search for
        the normalised sum, without the inputs>); (-1, -inf) where there is no row or an input id has no vector."""
        t = _i32(triples).reshape(-1, 3)
        Q = t.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        _check(self.lib.freddy_gpu_ivfadc_analogy(self.h, vecs.h, _p(t), Q, k, n_cand, W, C.c_float(sentinel), found_rule,
                                                  _p(out_i), _p(out_s)))
        return out_i, out_s

    def search_dev(self, d_queries_ptr, Q, k, W, sentinel, found_rule, d_out_ids_ptr, d_out_dist_ptr,
                   d_status_ptr=0, stream=None):
        _check(self.lib.freddy_gpu_ivfadc_search_dev(self.h, C.c_void_p(d_queries_ptr), Q, k, W,
                                                     C.c_float(sentinel), found_rule,
                                                     C.c_void_p(d_out_ids_ptr), C.c_void_p(d_out_dist_ptr),
                                                     C.c_void_p(d_status_ptr or 0), C.c_void_p(stream or 0)))

    def bind_search_dev(self, d_queries_ptr, Q, k, W, sentinel, found_rule, d_out_ids_ptr, d_out_dist_ptr,
                        d_status_ptr=0, stream=None):
        """search_dev with every argument converted ONCE: returns a zero-argument callable that makes the C call and
        raises on a non-zero status.  (A loop that enqueues the same batch again and again -- bench.py -- spent a
        quarter of its host time per step converting the eleven arguments.)"""
        fn = self.lib.freddy_gpu_ivfadc_search_dev
        args = (self.h, C.c_void_p(d_queries_ptr), C.c_int32(Q), C.c_int32(k), C.c_int32(W), C.c_float(sentinel),
                C.c_int32(found_rule), C.c_void_p(d_out_ids_ptr), C.c_void_p(d_out_dist_ptr),
                C.c_void_p(d_status_ptr or 0), C.c_void_p(stream or 0))

        def call():
            rc = fn(*args)
            if rc != 0:
                _check(rc)
        return call

    def last_scanned_rows(self):
        return int(self.lib.freddy_gpu_last_scanned_rows(self.h))

    def last_probed_cells(self):
        """(distinct cells, rows of their lists) of the last probing round (cell-grouped scans)."""
        n, r = C.c_int64(0), C.c_int64(0)
        _check(self.lib.freddy_gpu_last_probed_cells(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def coarse_bound_checked(self):
        return int(self.lib.freddy_gpu_coarse_bound_checked(self.h))

    def bound_checked(self):
        return int(self.lib.freddy_gpu_filter_bound_checked(self.h))


class IVPQIndex(_Index):
    """codebook_ivpq + coarse multi-index + fine_quantization_ivpq (+vectors, stats) in HBM."""
    kind = "ivpq"

    def __init__(self, codebook, coarse, ids, coarse_id, codes, vectors, stats, device=0):
        super().__init__()
        cb, cq, ids, cid, codes, st = (_f32(codebook), _f32(coarse), _i32(ids), _i32(coarse_id),
                                       _i16(codes), _f32(stats))
        vec = None if vectors is None else _f32(vectors)
        m, K, s = cb.shape
        cpos, ccodes, _ = cq.shape
        self.d, self.m, self.K, self.N = m * s, m, K, ids.size
        self.cells = ccodes * ccodes
        desc = IVPQDesc(self.d, m, K, cpos, ccodes, ids.size, _p(cb), _p(cq), _p(ids), _p(cid), _p(codes),
                        _p(vec), _p(st))
        _check(self.lib.freddy_gpu_pin_ivpq(C.byref(desc), device, C.byref(self.h)))

    def knn_join(self, queries, k, target_ids, alpha, pvf, method, use_target_lists=True, confidence=0.8,
                 double_threshold=10000000):
        qs = _f32(queries).reshape(-1, self.d)
        tid = _i32(target_ids)
        Q = qs.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_d = np.empty((Q, k), np.float32)
        iters = C.c_int32(0)
        _check(self.lib.freddy_gpu_knn_join(self.h, _p(qs), Q, k, _p(tid), tid.size, alpha, pvf, method,
                                            1 if use_target_lists else 0, C.c_float(confidence),
                                            double_threshold, _p(out_i), _p(out_d), C.byref(iters)))
        return out_i, out_d, iters.value

    def knn_join_ids(self, vecs, query_ids, k, target_ids, alpha, pvf, method, id_rule=QIDS_POSITIONAL, use_target_lists=True,
                     confidence=0.8, double_threshold=10000000):
        """knn_join() for the rows of the VectorIndex `vecs` -- None: of this handle's own pinned vectors -- with these ids, gathered
        on the device (freddy_gpu_knn_join_ids): (query_ids[Q], ids[Q,k], dist[Q,k], iterations) with Q = the queries `id_rule`
        selects; the lists of the ids that have a row and the iteration count are bit for bit ONE knn_join() over their vectors, a
        positional slot without a row holds (-1, 1000.0)."""
        tid = _i32(target_ids)
        iters = C.c_int32(0)
        oq, oi, od = _search_ids(query_ids, k, lambda q, n, oq, nq, oi, od: self.lib.freddy_gpu_knn_join_ids(
            self.h, None if vecs is None else vecs.h, _p(q), n, id_rule, k, _p(tid), tid.size, alpha, pvf, method, 1 if use_target_lists else 0,
            C.c_float(confidence), double_threshold, _p(oq), C.byref(nq), _p(oi), _p(od), C.byref(iters)))
        return oq, oi, od, iters.value

    def analogy(self, vecs, triples, k=1, n_cand=4, target_ids=(), alpha=1, pvf=1, method=METHOD_PQ, use_target_lists=True, confidence=0.8,
                double_threshold=10000000):
        """Approximate 3CosAdd analogies over the kNN-join (freddy_gpu_ivpq_analogy; analogy_3cosadd_in_ivpq with its literal
        n_cand = 4): triples [Q][3] of row ids -> (ids[Q,k], similarity[Q,k]); per triple bit for bit vecs.search(v3 - v1 + v2, k,
        subset_ids=<the ids of the join's list for the normalised sum, without the inputs>); (-1, -inf) where there is no row or an
        input id has no vector."""
        t = _i32(triples).reshape(-1, 3)
        Q = t.shape[0]
        out_i = np.empty((Q, k), np.int32)
        out_s = np.empty((Q, k), np.float32)
        tid = _i32(target_ids)
        _check(self.lib.freddy_gpu_ivpq_analogy(self.h, None if vecs is None else vecs.h, _p(t), Q, k, n_cand, _p(tid), tid.size, alpha, pvf, method,
                                                1 if use_target_lists else 0, C.c_float(confidence), double_threshold, _p(out_i), _p(out_s)))
        return out_i, out_s

    def set_statistics(self, stats):
        """set_statistics_table for the pinned handle (freddy_gpu_set_statistics): `stats` ([cells + 1] floats) becomes the row the
        kNN-join reads, on the device and on the host; nothing else of the handle changes."""
        st = _f32(stats).reshape(-1)
        _check(self.lib.freddy_gpu_set_statistics(self.h, _p(st), st.size))

    def statistics(self):
        """The statistics row the device holds (freddy_gpu_get_statistics): [cells + 1] floats."""
        out = np.empty(self.cells + 1, np.float32)
        _check(self.lib.freddy_gpu_get_statistics(self.h, _p(out), out.size))
        return out

    def create_statistics(self, ids=None, install=False):
        """create_statistics() over the pinned rows (freddy_gpu_create_statistics): ids = the row ids of a column's tokens, with
        their multiplicity (unknown ids are skipped); None = every pinned row once.  install=True makes the row the handle's row.
        -> (stats [cells + 1], matched = the entries that have a row)."""
        if ids is not None:
            ids = np.asarray(ids)
            if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
                raise FreddyGpuError("row ids are 32-bit integers")
            ids = _i32(ids).reshape(-1)
        n = 0 if ids is None else ids.size
        # (an empty LIST is not "every row": the library gets a pointer that is not NULL with n = 0 and refuses it)
        ptr = None if ids is None else _p(ids if n else np.zeros(1, np.int32))
        out = np.empty(self.cells + 1, np.float32)
        matched = C.c_int64(0)
        _check(self.lib.freddy_gpu_create_statistics(self.h, ptr, C.c_int64(n), 1 if install else 0, _p(out), C.byref(matched)))
        return out, int(matched.value)

    def last_track(self):
        """{stage name: seconds} of the most recent knn_join call (the reference's TRACK lines)."""
        t = Track()
        n = self.lib.freddy_gpu_last_track_sized(self.h, C.byref(t), C.sizeof(t))
        if n < 0:
            _check(n)
        return {n: getattr(t, n) for n, _ in Track._fields_}


class Track(C.Structure):
    """freddy_track: stage timers under the reference's TRACK names (ivpq_search_in.c:234-697)."""
    _fields_ = [("precomputation_time", C.c_double), ("determine_coarse_quantization_time", C.c_double),
                ("query_construction_time", C.c_double), ("data_retrieval_time", C.c_double),
                ("computation_time", C.c_double), ("pv_computation_time", C.c_double),
                ("recalculate_query_indices_time", C.c_double), ("total_time", C.c_double),
                ("join_kernel_time", C.c_double), ("candidate_rows", C.c_int64),
                ("iterations", C.c_int32), ("replay_us", C.c_int32), ("host_traversals", C.c_int64),
                ("libm_checks", C.c_int64)]


class EncodeDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("m", C.c_int32), ("K", C.c_int32), ("codebook", C.c_void_p), ("C", C.c_int32),
                ("coarse", C.c_void_p)]


def encode(codebook, vectors, coarse=None, device=0):
    """Index build, encoding step: (cell[N] or None, codes[N, m]) of `vectors` for a trained
    codebook [m][K][s] and optional coarse quantizer [C][d] (codes of the residuals then)."""
    lib = load()
    cb, v = _f32(codebook), _f32(vectors)
    m, K, s_ = cb.shape
    d = m * s_
    v = v.reshape(-1, d)
    co = None if coarse is None else _f32(coarse)
    desc = EncodeDesc(d, m, K, _p(cb), 0 if co is None else co.shape[0], _p(co))
    codes = np.empty((v.shape[0], m), np.int16)
    cell = None if co is None else np.empty(v.shape[0], np.int32)
    _check(lib.freddy_gpu_encode(C.byref(desc), device, _p(v), C.c_int64(v.shape[0]), _p(cell), _p(codes)))
    return cell, codes


class InsertDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("pq_m", C.c_int32), ("pq_K", C.c_int32), ("pq_codebook", C.c_void_p),
                ("res_m", C.c_int32), ("res_K", C.c_int32), ("residual_codebook", C.c_void_p),
                ("C", C.c_int32), ("coarse", C.c_void_p),
                ("ivpq_m", C.c_int32), ("ivpq_K", C.c_int32), ("ivpq_codebook", C.c_void_p),
                ("multi_positions", C.c_int32), ("multi_codes", C.c_int32), ("coarse_multi", C.c_void_p)]


def insert_quantize(vectors, pq_codebook=None, residual_codebook=None, coarse=None, ivpq_codebook=None, coarse_multi=None,
                    device=0):
    """insert_batch's quantisation of new vectors (freddy.c:1557-1623) on the device.  Returns a dict with the
    arrays of the parts that were given: pq_codes, coarse_id, residual_codes, ivpq_codes, coarse_multi_codes."""
    lib = load()
    v = _f32(vectors)
    n, d = v.shape
    keep = []

    def cb(a):
        if a is None:
            return 0, 0, None
        a = _f32(a)
        keep.append(a)
        return a.shape[0], a.shape[1], _p(a)

    pm, pk, pp = cb(pq_codebook)
    rm, rk, rp = cb(residual_codebook)
    im, ik, ip = cb(ivpq_codebook)
    mp, mk, mpp = cb(coarse_multi)
    co = None if coarse is None else _f32(coarse)
    desc = InsertDesc(d, pm, pk, pp, rm, rk, rp, 0 if co is None else co.shape[0], _p(co), im, ik, ip, mp, mk, mpp)
    out = {}
    if pp: out["pq_codes"] = np.empty((n, pm), np.int16)
    if rp:
        out["coarse_id"] = np.empty(n, np.int32)
        out["residual_codes"] = np.empty((n, rm), np.int16)
    if ip: out["ivpq_codes"] = np.empty((n, im), np.int16)
    if mpp: out["coarse_multi_codes"] = np.empty((n, mp), np.int16)
    _check(lib.freddy_gpu_insert_quantize(C.byref(desc), device, _p(v), C.c_int64(n), _p(out.get("pq_codes")), _p(out.get("coarse_id")),
                                          _p(out.get("residual_codes")), _p(out.get("ivpq_codes")), _p(out.get("coarse_multi_codes"))))
    return out


def kmeans(vectors, k, iters=10, init_rows=None, device=0):
    """Quantizer training on the device (quantizer_creation.py:13-52): (centroids[k, d], assignment[n])."""
    lib = load()
    v = _f32(vectors)
    cent = np.empty((int(k), v.shape[1]), np.float32)
    assign = np.empty(v.shape[0], np.int32)
    ir = None if init_rows is None else _i32(init_rows)
    _check(lib.freddy_gpu_kmeans(device, _p(v), C.c_int64(v.shape[0]), v.shape[1], int(k), int(iters), _p(ir), _p(cent), _p(assign)))
    return cent, assign


def train_pq_codebook(vectors, m, K, iters=10, seed=0, device=0):
    """create_quantizer (quantizer_creation.py:13-30): one k-means per sub-vector position -> [m][K][d/m]."""
    v = _f32(vectors)
    s_ = v.shape[1] // m
    rng = np.random.default_rng(seed)
    out = np.empty((m, K, s_), np.float32)
    for p in range(m):
        init = rng.choice(v.shape[0], K, replace=v.shape[0] < K).astype(np.int32)
        out[p], _ = kmeans(np.ascontiguousarray(v[:, p * s_:(p + 1) * s_]), K, iters, init, device)
    return out


class PinnedBuffer:
    """Pinned host memory from freddy_gpu_host_alloc as a numpy array: query batches written into it skip the
    staging copy of the host-buffer calls (include/freddy_gpu.h)."""

    def __init__(self, shape, dtype=np.float32):
        self.lib = load()
        self.ptr = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _check(self.lib.freddy_gpu_host_alloc(C.byref(self.ptr), n))
        buf = (C.c_char * max(n, 1)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.freddy_gpu_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
