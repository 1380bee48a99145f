"""The exact searches by row id and the device resolve's test hook exist in every layer: exported by libfreddy_gpu.so, declared in
include/freddy_gpu.h, listed and bound in freddy_amd/gpu.py.  No GPU: the library is loaded and inspected; only freddy_gpu_abi_version is called."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("freddy_gpu_exact_search_ids", "freddy_gpu_exact_join_ids", "freddy_gpu_debug_resolve_ids")


def test_the_library_exports_them():
    from freddy_amd import gpu
    lib = gpu.load()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes, n
    assert lib.freddy_gpu_abi_version() == 4


def test_the_header_declares_them_and_keeps_its_abi_version():
    h = open(os.path.join(ROOT, "include", "freddy_gpu.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(freddy_gpu_index_t\* vecs, const int32_t\* (query_ids|ids),", h), n
    for n in NAMES[:2]:
        m = re.search(r"int " + n + r"\(([^;]*)\);", h)
        args = re.sub(r"/\*.*?\*/", "", m.group(1))
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == \
            ["vecs", "query_ids", "n_ids", "id_rule", "k", "subset_ids" if "search" in n else "target_ids",
             "n_subset" if "search" in n else "n_targets", "out_query_ids", "n_queries", "out_ids", "out_sim"], n
    assert "#define FREDDY_GPU_ABI_VERSION 4" in h
    for opt in ('"exact_resolve"', '"resolve_block"'):
        assert opt in h, opt


def test_the_binding_lists_and_wraps_them():
    from freddy_amd import gpu
    for n in NAMES:
        assert n in gpu.EXPORTS, n
    for m in ("exact_search_ids", "exact_join_ids", "debug_resolve_ids"):
        assert callable(getattr(gpu.VectorIndex, m, None)), m
    assert gpu.ABI_VERSION == 4
