"""CPU suite for the batched approximate analogies (approx_analogy.h; freddy_gpu_ivfadc_analogy / freddy_gpu_pq_analogy /
freddy_gpu_last_approx_analogy_stats; the host mirror's analogy_3cosadd_*_batch): the model of tests/approx_analogy_model.py against
a literal restatement of analogy_common's host loop, the properties the GPU tests' triples must have, declared / exported / listed
symbols, every argument and limit error that needs no device, and a codegen guard for the two new kernels (0 spilled registers,
0 scratch).  Handles of the wrong kind, of another d or with replicas cannot exist without a device: tests/test_gpu_approx_analogy.py."""
import ctypes
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
GPU_SYMBOLS = ("freddy_gpu_ivfadc_analogy", "freddy_gpu_pq_analogy", "freddy_gpu_last_approx_analogy_stats")
UDF_SYMBOLS = ("analogy_3cosadd_pq_batch", "analogy_3cosadd_ivfadc_batch", "analogy_3cosadd_in_pq_batch", "freddy_session_gpu_index")


def test_model_equals_the_host_loop_of_analogy_common(oracle):
    """A 2000 x 24 table whose rows 1000..1039 are copies of rows 20..59, IVFADC, flat PQ and subset PQ lists at n_cand = 23 (pvf = 20);
    the vector table lacks every seventh id.  The model's first row (oracle search -> drop -> oracle exact_knn at k = 1) equals
    analogy_common's loop, id and similarity bits; a triple with an id that has no vector has no rows and is not counted."""
    import approx_analogy_model as am
    import util
    from freddy_amd import index_build as ib
    N, d, n_cand = 2000, 24, 23
    x = util.shape_corpus(N, d).numpy().copy()
    x[1000:1040] = x[20:60]
    ids = np.arange(1, N + 1, dtype=np.int32)
    xt = torch.from_numpy(x)
    ivf = ib.build_ivf_index(xt, C=8, m=4, K=16, train_size=N, iters=3, seed=1)
    pq = ib.build_pq_index(xt, m=4, K=16, train_size=N, iters=3, seed=2)
    keep = ids % 7 != 0
    vx, vids = x[keep], ids[keep]
    rng = np.random.default_rng(4)
    t = rng.choice(ids, (120, 3)).astype(np.int32)
    t[:20, 2] = t[:20, 0]                                   # w1 == w3: raw is v2 exactly
    t[20:40, 1] = ids[20:40]                                # ... and v2 a duplicated row
    t[20:40, 2] = t[20:40, 0]
    t[60] = (5, 10**6, 9)                                   # unknown ids
    t[61] = (-3, 8, 9)
    it = oracle.ivf_table(ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    pt = oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])
    sub = np.concatenate([ids[10:1500], ids[10:30], np.array([-4, 10**6], np.int32)])
    n_invalid = int((~np.isin(t, vids)).any(axis=1).sum())
    assert n_invalid > 10
    excluded = 0
    for res in (am.ivf_expected(oracle, it, vx, vids, t, 1, n_cand, 2), am.pq_expected(oracle, pt, vx, vids, t, 1, n_cand),
                am.pq_expected(oracle, pt, vx, vids, t, 1, n_cand, sub)):
        exp, st, lists, raw, valid = res
        assert st["searched"] == len(t) - n_invalid == len(lists) and 0 < st["scored"] < st["candidates"] <= lists.size
        j = 0
        for q in range(len(t)):
            if not valid[q]:
                assert len(exp[q]) == 0 and am.analogy_loop(vx, vids, t[q], np.arange(1, 24)) == (-1, None)
                continue
            got_id, got_sim = am.analogy_loop(vx, vids, t[q], lists[j])
            excluded += int(np.isin(t[q], lists[j]).any())
            assert [got_id] == exp[q]["id"].tolist(), q
            assert np.float32(got_sim).view(np.uint32) == exp[q]["dist"].view(np.uint32)[0], q
            j += 1
    assert excluded > 0, "no list ever held an input id"
    # k > 1: the rows are those of exact_knn over the kept candidates, in its order; every list entry without a vector or equal to an input is gone
    exp, st, lists, raw, valid = am.ivf_expected(oracle, it, vx, vids, t, 8, 40, 2)
    ties = 0
    for q, e in zip(np.flatnonzero(valid), (e for e, v in zip(exp, valid) if v)):
        assert not np.isin(e["id"], t[q]).any() and np.isin(e["id"], vids).all()
        assert (np.diff(e["dist"]) <= 0).all()
        ties += int(((np.diff(e["dist"]) == 0) & (np.diff(e["id"]) > 0)).sum())
    assert ties > 0, "no two answers ever tied: the duplicate rows never met in a list"


def test_the_main_case_triples_have_the_properties_the_gpu_tests_need(oracle):
    """On the model's data, at every (k, n_cand) of the GPU main case: some triple has an input id among its stage-one candidates and
    would be answered by that input without the exclusion; some triple's two best answers have equal similarity (a duplicate pair), so
    the id order decides even at k = 1; some triple repeats an id."""
    import approx_analogy_model as am
    import pv_model as pm
    x, ids, _, ivf, _ = pm.main_tables()
    t = am.main_triples()
    assert t.shape == (200, 3) and (t[:, 0] == t[:, 2]).sum() >= 10
    it = oracle.ivf_table(ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    for k, n_cand in ((1, 4), (1, 23), (5, 64), (5, 65), (32, 640)):
        exp, st, lists, raw, valid = am.ivf_expected(oracle, it, x, ids, t, k, n_cand, 3)
        assert valid.all()
        decides = top_ties = 0
        for q in range(200):
            _, have = pm.candidates(lists[q], ids)
            with_inputs = pm.rerank(oracle, x, ids, raw[q], 1, have)
            decides += int(len(with_inputs) and int(with_inputs["id"][0]) in t[q].tolist())
            two = pm.rerank(oracle, x, ids, raw[q], 2, have[~np.isin(have, t[q])])
            top_ties += int(len(two) == 2 and two["dist"][0] == two["dist"][1])
        assert decides > 0 and top_ties > 0, (k, n_cand, decides, top_ties)
        assert st["scored"] < st["candidates"]


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
        assert hasattr(cls, "analogy") and hasattr(cls, "last_approx_analogy_stats"), cls
    for n in ("analogy_3cosadd_pq_batch", "analogy_3cosadd_ivfadc_batch", "analogy_3cosadd_in_pq_batch", "gpu_index"):
        assert hasattr(udf.Session, n), n
    assert "analogy_3cosadd_in_ivpq_batch" not in uh                # out of scope: the kNN-join with the literal k = 4


def test_argument_and_limit_errors_without_a_gpu():
    """Sizes, W, found_rule, the subset, NULL buffers and the 4096-candidate limit are reported before the handles are looked at
    (FREDDY_E_ARG = -1, FREDDY_E_LIMIT = -5, each with the offending value in the message); NULL handles are FREDDY_E_ARG."""
    from freddy_amd import gpu
    lib = gpu.load()
    t = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    oi = np.empty(2 * 4096, np.int32)
    os_ = np.empty(2 * 4096, np.float32)
    sub = np.array([1, 2, 3], np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    err = lib.freddy_gpu_last_error
    f = ctypes.c_float

    def ivf(Q, k, n_cand, W=3, tp=P(t), ip=P(oi), sp=P(os_), rule=0):
        return lib.freddy_gpu_ivfadc_analogy(None, None, tp, Q, k, n_cand, W, f(1000.0), rule, ip, sp)

    def pq(Q, k, n_cand, subp=None, ns=0, tp=P(t), ip=P(oi), sp=P(os_)):
        return lib.freddy_gpu_pq_analogy(None, None, tp, Q, k, n_cand, f(100.0), subp, ns, ip, sp)

    for call in (ivf, pq):
        assert call(2, 0, 4) == -1 and b"bad sizes" in err() and b"k=0" in err()
        assert call(2, -3, 4) == -1 and b"k=-3" in err()
        assert call(2, 5, 4) == -1 and b"bad sizes" in err() and b"n_cand=4" in err()           # n_cand < k
        assert call(-1, 1, 4) == -1 and b"bad sizes" in err() and b"Q=-1" in err()
        assert call(2, 1, 4, tp=None) == -1 and b"NULL buffer" in err()
        assert call(2, 1, 4, ip=None) == -1 and b"NULL buffer" in err()
        assert call(2, 1, 4, sp=None) == -1 and b"NULL buffer" in err()
        assert call(2, 1, 4097) == -5 and b"n_cand = 4097 exceeds this build's limit of 4096 candidates" in err()
        assert call(2, 64, 2**30) == -5 and b"n_cand = 1073741824 " in err()
        assert call(2, 64, 4096) == -1 and b"NULL index" in err()                               # 4096 itself is within the limit
        assert call(2, 1, 1) == -1 and b"NULL index" in err()                                   # n_cand == k is allowed
        assert call(0, 1, 4, tp=None, ip=None, sp=None) == -1 and b"NULL index" in err()        # Q = 0 needs no buffers, but handles
    assert ivf(2, 1, 4, W=0) == -1 and b"W must be positive" in err()
    assert ivf(2, 1, 4, W=-2) == -1 and b"W must be positive" in err()
    assert ivf(2, 1, 4, rule=3) == -1 and b"bad found_rule" in err()
    assert ivf(2, 1, 4, rule=-1) == -1 and b"bad found_rule" in err()
    assert ivf(2, 1, 4, W=3, rule=2) == -1 and b"FREDDY_FOUND_BATCH_UDF needs W == 1" in err()
    assert pq(2, 1, 4, None, 3) == -1 and b"bad subset" in err() and b"n_subset=3" in err()
    assert pq(2, 1, 4, P(sub), -1) == -1 and b"n_subset=-1" in err()
    assert lib.freddy_gpu_last_approx_analogy_stats(None, None, None, None) == -1 and b"NULL index" in err()


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    t = [[1, 2, 3], [4, 5, 6]]
    with pytest.raises(udf.FreddyError, match="coarse_quantization / residual_codebook / fine_quantization are not loaded"):
        s.analogy_3cosadd_ivfadc_batch(t)
    with pytest.raises(udf.FreddyError, match="pq_quantization / pq_codebook are not loaded"):
        s.analogy_3cosadd_pq_batch(t)
    with pytest.raises(udf.FreddyError, match="pq_quantization / pq_codebook are not loaded"):
        s.analogy_3cosadd_in_pq_batch(t, [1, 2, 3])
    out = np.empty(2, np.int32)
    assert s.lib.analogy_3cosadd_pq_batch(s.h, None, 2, out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert s.lib.freddy_udf_last_error() == b"bad argument"
    assert s.gpu_index("pq") is None and s.gpu_index("vecs") is None and s.gpu_index("no such table") is None
    s.close()


# ---- codegen guard -------------------------------------------------------------------------------------------------------
PROBES = {
    "aa_query_kernel": ("aa_query_kernel", "aa_query_kernel"),
    "aa_rerank_kernel<1>": ("aa_rerank_kernel<1>", "aa_rerank_kernelILi1EE"),
    "aa_rerank_kernel<4>": ("aa_rerank_kernel<4>", "aa_rerank_kernelILi4EE"),
}
FIELDS = {"ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "aa_probe.hip")
    with open(src, "w") as f:
        f.write('#include "pv.h"\n#include "approx_analogy.h"\nusing namespace freddy;\nconst void* probe_kernels[] = {'
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
def test_the_new_kernels_do_not_spill(tmp_path):
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill", "sgpr_spill") if g[k]]
    assert not bad, "\n".join(bad)
