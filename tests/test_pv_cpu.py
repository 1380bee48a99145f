"""CPU suite for the batched post verification (pv.h; freddy_gpu_ivfadc_search_pv / freddy_gpu_pq_search_pv / freddy_gpu_last_pv_stats;
the host mirror's k_nearest_neighbour_*_pv_batch and knn_batch()): the model of tests/pv_model.py against a literal restatement of
knn_pv's loop, declared / exported / listed symbols, every argument and limit error that needs no device, and a codegen guard for
the pv_ kernels (0 spilled VGPRs, 0 scratch; VGPRs and SGPRs within tests/golden/pv_codegen_ceilings.json).  Handles of the wrong
kind, of another d or with replicas cannot exist without a device: tests/test_gpu_pv.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
CEILINGS = os.path.join(ROOT, "tests", "golden", "pv_codegen_ceilings.json")
GPU_SYMBOLS = ("freddy_gpu_ivfadc_search_pv", "freddy_gpu_pq_search_pv", "freddy_gpu_last_pv_stats")
UDF_SYMBOLS = ("k_nearest_neighbour_ivfadc_pv_batch", "k_nearest_neighbour_pq_pv_batch", "freddy_set_knn_batch_function",
               "freddy_get_knn_batch_function", "knn_batch")


def test_model_equals_the_host_loop_of_knn_pv(oracle):
    """A 600 x 24 table whose rows 300..339 are copies of rows 20..59, IVFADC and flat PQ lists at k * pvf = 40; the vector table
    lacks every third id.  The model's lists (oracle search -> drop -> oracle exact_knn) equal knn_pv's loop, ids and bits."""
    import pv_model as pm
    import util
    from freddy_amd import index_build as ib
    N, d = 600, 24
    x = util.shape_corpus(N, d).numpy().copy()
    x[300:340] = x[20:60]
    ids = np.arange(1, N + 1, dtype=np.int32)
    xt = torch.from_numpy(x)
    ivf = ib.build_ivf_index(xt, C=4, m=4, K=16, train_size=N, iters=3, seed=1)
    pq = ib.build_pq_index(xt, m=4, K=16, train_size=N, iters=3, seed=2)
    keep = ids % 3 != 0
    vx, vids = x[keep], ids[keep]
    qs = np.concatenate([x[20:30], -x[40:42], x[::97]])
    it = oracle.ivf_table(ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    pt = oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])
    sub = np.concatenate([ids[10:400], ids[10:30], np.array([-4, 10**6], np.int32)])
    ties = 0
    for lists in (pm.ivf_lists(oracle, it, qs, 40, 2), pm.pq_lists(oracle, pt, qs, 40), pm.pq_lists(oracle, pt, qs, 40, sub)):
        exp, n_cand, n_scored = pm.expected(oracle, lists, vx, vids, qs, 8)
        assert 0 < n_scored.sum() < n_cand.sum() <= lists.size
        for q, l, e in zip(qs, lists, exp):
            loop = pm.knn_pv_loop(vx, vids, q, 8, l)
            assert [c[0] for c in loop] == e["id"].tolist()
            assert np.array_equal(np.array([c[1] for c in loop], np.float32).view(np.uint32), e["dist"].view(np.uint32))
            ties += int((np.diff(e["dist"]) == 0).sum())
    assert ties > 0, "no two candidates ever tied: the duplicate rows never met in a list"
    # an empty candidate set is an empty list
    exp, n_cand, n_scored = pm.expected(oracle, np.full((1, 40), -1, np.int32), vx, vids, qs[:1], 8)
    assert len(exp[0]) == 0 and (n_cand.sum(), n_scored.sum()) == (0, 0)
    exp, n_cand, n_scored = pm.expected(oracle, np.full((1, 40), 3, np.int32), vx, vids, qs[:1], 8)   # id 3 has no vector
    assert len(exp[0]) == 0 and (n_cand.sum(), n_scored.sum()) == (40, 0)


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
    for cls in (gpu.IVFIndex, gpu.PQIndex):
        assert hasattr(cls, "search_pv") and hasattr(cls, "last_pv_stats"), cls
    for n in ("k_nearest_neighbour_ivfadc_pv_batch", "k_nearest_neighbour_pq_pv_batch", "knn_batch", "set_knn_batch_function",
              "get_knn_batch_function_name"):
        assert hasattr(udf.Session, n), n


def test_argument_and_limit_errors_without_a_gpu():
    """Sizes, NULL buffers and the 4096-candidate limit are reported before the handles are looked at: FREDDY_E_ARG = -1,
    FREDDY_E_LIMIT = -5, each with the offending value in the message."""
    from freddy_amd import gpu
    lib = gpu.load()
    q = np.zeros((2, 8), np.float32)
    oi = np.empty(2 * 4096, np.int32)
    os_ = np.empty(2 * 4096, np.float32)
    sub = np.array([1, 2, 3], np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    err = lib.freddy_gpu_last_error
    f = ctypes.c_float

    def ivf(Q, k, pvf, W=3, qp=P(q), ip=P(oi), sp=P(os_), rule=0):
        return lib.freddy_gpu_ivfadc_search_pv(None, None, qp, Q, k, pvf, W, f(1000.0), rule, ip, sp)

    def pq(Q, k, pvf, subp=None, ns=0, qp=P(q), ip=P(oi), sp=P(os_)):
        return lib.freddy_gpu_pq_search_pv(None, None, qp, Q, k, pvf, f(100.0), subp, ns, ip, sp)

    for call in (ivf, pq):
        assert call(2, 0, 4) == -1 and b"bad sizes" in err() and b"k=0" in err()
        assert call(2, -3, 4) == -1 and b"k=-3" in err()
        assert call(2, 5, 0) == -1 and b"bad sizes" in err() and b"pvf=0" in err()
        assert call(2, 5, -2) == -1 and b"pvf=-2" in err()
        assert call(-1, 5, 4) == -1 and b"bad sizes" in err() and b"Q=-1" in err()
        assert call(2, 5, 4, qp=None) == -1 and b"NULL buffer" in err()
        assert call(2, 5, 4, ip=None) == -1 and b"NULL buffer" in err()
        assert call(2, 5, 4, sp=None) == -1 and b"NULL buffer" in err()
        assert call(2, 64, 65) == -5 and b"k * pvf = 4160 exceeds this build's limit of 4096 candidates" in err()
        assert call(2, 4097, 1) == -5 and b"k * pvf = 4097 " in err()
        assert call(2, 2**20, 2**20) == -5 and b"k * pvf = 1099511627776 " in err()          # (no 32-bit overflow of the product)
        assert call(2, 64, 64) == -1 and b"NULL index" in err()                              # 4096 itself is within the limit
        assert call(0, 5, 4, qp=None, ip=None, sp=None) == -1 and b"NULL index" in err()     # Q = 0 needs no buffers, but handles
    assert pq(2, 5, 4, None, 3) == -1 and b"bad subset" in err() and b"n_subset=3" in err()
    assert pq(2, 5, 4, P(sub), -1) == -1 and b"n_subset=-1" in err()
    assert lib.freddy_gpu_last_pv_stats(None, None, None) == -1 and b"NULL index" in err()


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    assert s.get_knn_batch_function_name() == "k_nearest_neighbour_ivfadc_batch"
    with pytest.raises(udf.FreddyError, match="coarse_quantization / residual_codebook / fine_quantization are not loaded"):
        s.k_nearest_neighbour_ivfadc_pv_batch([1, 2], 5)
    with pytest.raises(udf.FreddyError, match="pq_quantization / pq_codebook are not loaded"):
        s.k_nearest_neighbour_pq_pv_batch([1, 2], 5)
    with pytest.raises(udf.FreddyError, match="not loaded"):
        s.knn_batch([1, 2], 5)
    for name, arm in (("k_nearest_neighbour_ivfadc_pv_batch", "coarse_quantization"), ("k_nearest_neighbour_pq_pv_batch", "pq_quantization")):
        s.set_knn_batch_function(name)
        assert s.get_knn_batch_function_name() == name
        with pytest.raises(udf.FreddyError, match=arm):
            s.knn_batch([1, 2], 5)
    s.set_knn_batch_function("k_nearest_neighbour_typo")          # the setter accepts any name; the call fails
    assert s.get_knn_batch_function_name() == "k_nearest_neighbour_typo"
    with pytest.raises(udf.FreddyError, match=r"^function k_nearest_neighbour_typo\(character varying\[\], integer\) does not exist$"):
        s.knn_batch([1, 2], 5)
    s.close()


# ---- codegen guard -------------------------------------------------------------------------------------------------------
PROBES = {
    "pv_rerank_kernel<1>": ("pv_rerank_kernel<1>", "pv_rerank_kernelILi1EE"),
    "pv_rerank_kernel<4>": ("pv_rerank_kernel<4>", "pv_rerank_kernelILi4EE"),
}
FIELDS = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "pv_probe.hip")
    with open(src, "w") as f:
        f.write('#include "pv.h"\nusing namespace freddy;\nconst void* probe_kernels[] = {'
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
def test_pv_kernels_do_not_spill(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill") if g[k]]
    for name, g in got.items():
        for k in ("vgprs", "sgprs", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            if g[k] > ceilings[name][k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {ceilings[name][k]}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_pv_cpu.py [--write]: print (and commit) today's figures
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
