"""The searches by row id (include/freddy_gpu.h: freddy_gpu_*_search_ids) are declared, exported and bound, and report their
argument errors without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["freddy_gpu_ivfadc_search_ids", "freddy_gpu_pq_search_ids", "freddy_gpu_ivfadc_search_pv_ids", "freddy_gpu_pq_search_pv_ids"]


def _lib():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu
    return gpu, gpu.load()


def test_the_four_symbols_are_declared_exported_and_bound():
    gpu, lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "freddy_gpu.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, hdr), f"{n} is not declared"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in gpu.EXPORTS and getattr(lib, n).argtypes, n
    assert re.search(r"#define FREDDY_QIDS_TABLE_ORDER 0\b", hdr) and re.search(r"#define FREDDY_QIDS_POSITIONAL 1\b", hdr)
    assert (gpu.QIDS_TABLE_ORDER, gpu.QIDS_POSITIONAL) == (0, 1)
    assert lib.freddy_gpu_abi_version() == 4 and "#define FREDDY_GPU_ABI_VERSION 4" in hdr
    for cls in (gpu.IVFIndex, gpu.PQIndex):
        assert callable(cls.search_ids) and callable(cls.search_pv_ids)


def test_argument_errors_are_reported_without_a_gpu():
    gpu, lib = _lib()
    nq = C.c_int32(7)
    buf = (C.c_int32 * 8)()
    f = C.c_float
    calls = {
        "freddy_gpu_ivfadc_search_ids": lambda a, v: lib.freddy_gpu_ivfadc_search_ids(a, v, buf, 1, 0, 5, 3, f(1000.0), 0, buf, C.byref(nq), buf, buf),
        "freddy_gpu_pq_search_ids": lambda a, v: lib.freddy_gpu_pq_search_ids(a, v, buf, 1, 0, 5, f(100.0), None, 0, buf, C.byref(nq), buf, buf),
        "freddy_gpu_ivfadc_search_pv_ids": lambda a, v: lib.freddy_gpu_ivfadc_search_pv_ids(a, v, buf, 1, 0, 5, 2, 3, f(1000.0), 0, buf, C.byref(nq), buf, buf),
        "freddy_gpu_pq_search_pv_ids": lambda a, v: lib.freddy_gpu_pq_search_pv_ids(a, v, buf, 1, 0, 5, 2, f(100.0), None, 0, buf, C.byref(nq), buf, buf),
    }
    for name, call in calls.items():
        assert call(None, None) == -1, name
        assert b"NULL index" in lib.freddy_gpu_last_error(), name
        assert nq.value == 7, name                    # a refused call writes nothing
