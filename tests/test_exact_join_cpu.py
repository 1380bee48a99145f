"""CPU suite for the exact kNN-join (exact_join.h, freddy_gpu_exact_join, the host mirror's knn_search_in_batch / grouping_func /
groups()): declared and exported symbols, argument / limit errors without a GPU, and a codegen guard for the new kernels (0 VGPR
spills, 0 scratch; VGPRs and SGPR spills within the committed ceilings).  A handle of another kind cannot exist without a device:
that error is checked in tests/test_gpu_exact_join.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
CEILINGS = os.path.join(ROOT, "tests", "golden", "exact_join_codegen_ceilings.json")
GPU_SYMBOLS = ("freddy_gpu_exact_join", "freddy_gpu_last_exact_join_stats")
UDF_SYMBOLS = ("knn_search_in_batch", "knn_search_in_batch_ids", "grouping_func", "freddy_set_groups_function", "freddy_get_groups_function", "groups")


def _decl(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_symbols_are_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu, udf
    gh, uh = _decl("freddy_gpu.h"), _decl("freddy_udf.h")
    for n in GPU_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", gh), n
        assert hasattr(gpu.load(), n), n
        assert n in gpu.EXPORTS, n
    lib = udf.load()
    for n in UDF_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", uh), n
        assert hasattr(lib, n), n
    assert hasattr(gpu.VectorIndex, "join") and hasattr(gpu.VectorIndex, "last_join_stats")
    for n in ("knn_search_in_batch", "knn_search_in_batch_ids", "grouping_func", "groups", "set_groups_function", "get_groups_function_name"):
        assert hasattr(udf.Session, n), n


def test_argument_and_limit_errors_without_a_gpu():
    from freddy_amd import gpu
    lib = gpu.load()
    q = np.zeros((2, 8), np.float32)
    t = np.array([1, 2, 3], np.int32)
    oi = np.empty(2 * 4096, np.int32)
    os_ = np.empty(2 * 4096, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    call = lambda ix, Q, k, tp, nt, qp=P(q), ip=P(oi), sp=P(os_): lib.freddy_gpu_exact_join(ix, qp, Q, k, tp, nt, ip, sp)   # noqa: E731
    err = lib.freddy_gpu_last_error
    # sizes and limits are reported before the handle is looked at (no device work): FREDDY_E_ARG = -1, FREDDY_E_LIMIT = -5
    assert call(None, 2, 0, P(t), 3) == -1 and b"bad sizes" in err() and b"k=0" in err()
    assert call(None, 2, -3, P(t), 3) == -1 and b"bad sizes" in err()
    assert call(None, -1, 5, P(t), 3) == -1 and b"bad sizes" in err()
    assert call(None, 2, 5, P(t), -1) == -1 and b"bad sizes" in err()
    assert call(None, 2, 4097, P(t), 3) == -5 and b"k=4097 exceeds this build's limit of 4096" in err()
    assert call(None, 2, 5, None, 3) == -1 and b"NULL target_ids with n_targets=3" in err()
    assert call(None, 2, 5, P(t), 3, qp=None) == -1 and b"NULL buffer" in err()
    assert call(None, 2, 5, P(t), 3, ip=None) == -1 and call(None, 2, 5, P(t), 3, sp=None) == -1
    assert call(None, 2, 4096, P(t), 3) == -1 and b"NULL index" in err()            # k = 4096 is within the limit
    assert call(None, 2, 5, None, 0) == -1 and b"NULL index" in err()               # NULL targets with n_targets == 0: the empty set
    assert lib.freddy_gpu_last_exact_join_stats(None, None, None, None) == -1 and b"NULL index" in err()


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    q = np.zeros((2, 8), np.float32)
    assert s.get_groups_function_name() == "grouping_func"
    for call in (lambda: s.knn_search_in_batch(q, 5, [1, 2]), lambda: s.knn_search_in_batch_ids([1, 2], 5, [1, 2]),
                 lambda: s.grouping_func([1, 2], [3]), lambda: s.groups([1, 2], [3])):
        with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
            call()
    s.load_vecs_norm(np.arange(1, 5, dtype=np.int32), np.ones((4, 12), np.float32))
    with pytest.raises(udf.FreddyError, match="^query has 8 dimensions, table has 12$"):
        s.knn_search_in_batch(q, 5, [1, 2])
    q12 = np.zeros((2, 12), np.float32)
    with pytest.raises(udf.FreddyError, match="bad argument"):
        s.knn_search_in_batch(q12, 0, [1, 2])
    with pytest.raises(udf.FreddyError, match="^k=4097 exceeds this build's limit of 4096$"):
        s.knn_search_in_batch(q12, 4097, [1, 2])
    with pytest.raises(udf.FreddyError, match="^k=4097 exceeds this build's limit of 4096$"):
        s.knn_search_in_batch_ids([1, 2], 4097, [1, 2])
    # NULL input_ids with n_ids > 0 (the binding never passes one: straight through the C ABI)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    out3, outg, n = np.empty(16, udf.ROW3), np.empty(16, udf.GROUP_ROW), ctypes.c_int32(0)
    ids = np.array([1, 2], np.int32)
    for rc in (s.lib.knn_search_in_batch(s.h, P(q12), 2, 12, 5, None, 3, P(out3), ctypes.byref(n)),
               s.lib.knn_search_in_batch_ids(s.h, P(ids), 2, 5, None, 3, P(out3), ctypes.byref(n)),
               s.lib.grouping_func(s.h, P(ids), 2, None, 3, P(outg), ctypes.byref(n)),
               s.lib.grouping_func(s.h, None, 2, P(ids), 2, P(outg), ctypes.byref(n))):
        assert rc == -1 and s.lib.freddy_udf_last_error() == b"bad argument"
    s.set_groups_function("grouping_func_typo")                  # the setter accepts any name; the call fails
    assert s.get_groups_function_name() == "grouping_func_typo"
    with pytest.raises(udf.FreddyError, match=r"^function grouping_func_typo\(character varying\[\], character varying\[\]\) does not exist$"):
        s.groups([1, 2], [3])
    s.close()


# ---- codegen guard -------------------------------------------------------------------------------------------------------
PROBES = {
    "exj_filter_kernel<4,false>": ("exj_filter_kernel<4, false>", "exj_filter_kernelILi4ELb0EE"),
    "exj_filter_kernel<2,false>": ("exj_filter_kernel<2, false>", "exj_filter_kernelILi2ELb0EE"),
    "exj_filter_kernel<4,true>": ("exj_filter_kernel<4, true>", "exj_filter_kernelILi4ELb1EE"),
    "exj_gather_kernel": ("exj_gather_kernel", "17exj_gather_kernelE"),
}
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "exj_probe.hip")
    with open(src, "w") as f:
        f.write('#include "exact_join.h"\nusing namespace freddy;\nconst void* probe_kernels[] = {'
                + ", ".join(f"(const void*)&{inst}" for inst, _ in PROBES.values()) + "};\n")
    cmd = [os.environ.get("HIPCC", "hipcc")] + flags + ["-I" + CSRC, "-c", "-o", src[:-4] + ".o", src, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    got, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = next((n for n, (_, mangled) in PROBES.items() if mangled in m.group(1)), None)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if cur and m and m.group(1).strip() in FIELDS:
            got.setdefault(cur, {})[FIELDS[m.group(1).strip()]] = int(m.group(2))
    assert set(got) == set(PROBES), f"resource remarks not found for {set(PROBES) - set(got)}"
    return got


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc not on PATH")
def test_exact_join_kernels_do_not_spill(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill") if g[k]]
    for name, g in got.items():
        for k in ("vgprs", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            if g[k] > ceilings[name][k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {ceilings[name][k]}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_exact_join_cpu.py [--write]: print (and commit) today's figures
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
