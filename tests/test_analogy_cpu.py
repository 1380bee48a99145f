"""CPU suite for the exact analogies (analogy.h, freddy_gpu_exact_analogy, the host mirror's analogy functions): exported
symbols, argument / limit errors without a GPU, the numpy model (tests/analogy_model.py) against the oracle's
cosine_similarity_bytea / vec_minus / vec_plus, and a codegen guard for the new kernels (0 VGPR spills, 0 scratch; SGPR spills, which
go to VGPR lanes, within the committed ceilings)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import analogy_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
CEILINGS = os.path.join(ROOT, "tests", "golden", "analogy_codegen_ceilings.json")


def test_new_symbols_are_exported():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu, udf
    assert hasattr(gpu.load(), "freddy_gpu_exact_analogy") and hasattr(gpu.load(), "freddy_gpu_last_analogy_stats")
    lib = udf.load()
    for n in ("analogy_3cosadd", "analogy_3cosadd_in", "analogy_3cosmul", "analogy", "analogy_in", "freddy_set_analogy_function",
              "freddy_get_analogy_function", "freddy_set_analogy_in_function", "freddy_get_analogy_in_function"):
        assert hasattr(lib, n), n


def test_argument_and_limit_errors_without_a_gpu():
    from freddy_amd import gpu
    lib = gpu.load()
    t = np.array([[1, 2, 3]], np.int32)
    oi = np.empty(40, np.int32)
    os_ = np.empty(40, np.float64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    call = lambda ix, m, Q, k, sub=None, ns=0: lib.freddy_gpu_exact_analogy(ix, m, P(t), Q, k, sub, ns, P(oi), P(os_))   # noqa: E731
    assert call(None, 0, 1, 33) == -5 and b"33" in lib.freddy_gpu_last_error()        # FREDDY_E_LIMIT, k > 32
    assert call(None, 2, 1, 1) == -1                                                     # unknown method
    assert call(None, 1, -1, 1) == -1 and call(None, 1, 1, 0) == -1                      # bad sizes
    assert call(None, 1, 1, 1, None, 5) == -1                                            # a subset count without ids
    assert lib.freddy_gpu_exact_analogy(None, 0, None, 1, 1, None, 0, P(oi), P(os_)) == -1   # NULL triples
    assert call(None, 1, 1, 1) == -1 and b"NULL index" in lib.freddy_gpu_last_error()
    assert lib.freddy_gpu_last_analogy_stats(None, None, None, None) == -1


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    assert s.get_analogy_function_name() == "analogy_3cosadd" and s.get_analogy_in_function_name() == "analogy_3cosadd_in"
    with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
        s.analogy(1, 2, 3)                                       # the default: analogy_3cosadd
    with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
        s.analogy_3cosmul(1, 2, 3)
    s.set_analogy_function("analogy_3cosmul_typo")               # the setter accepts any name; the call fails
    assert s.get_analogy_function_name() == "analogy_3cosmul_typo"
    with pytest.raises(udf.FreddyError, match=r"^function analogy_3cosmul_typo\(unknown, unknown, unknown\) does not exist$"):
        s.analogy(1, 2, 3)
    s.set_analogy_in_function("analogy_3cosmul")                 # exists, but not with four arguments
    with pytest.raises(udf.FreddyError, match=r"^function analogy_3cosmul\(unknown, unknown, unknown, character varying\[\]\) does not exist$"):
        s.analogy_in(1, 2, 3, [4, 5])
    s.close()


def test_model_equals_oracle_compositions(oracle):
    """The model's float32 chains, 3CosAdd raw vector and float8 3CosMul combination equal compositions of the oracle's
    cosine_similarity_bytea / vec_minus / vec_plus bit for bit."""
    rng = np.random.default_rng(0)
    d, N = 300, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    x[5] *= np.float32(3.5)                                        # not every row normalised
    x_t = np.ascontiguousarray(x.T)
    for w1, w2, w3 in ((1, 2, 3), (7, 7, 9), (5, 11, 5)):
        raw = am.raw_3cosadd(x[w1], x[w2], x[w3])
        assert np.array_equal(raw.view(np.uint32), oracle.vec_plus(oracle.vec_minus(x[w3], x[w1]), x[w2]).view(np.uint32))
        add = am.scores(x, x_t, [(w1, w2, w3)], "3cosadd")[0]
        mul = am.scores(x, x_t, [(w1, w2, w3)], "3cosmul")[0]
        for r in range(0, N, 7):
            assert add[r] == np.float64(oracle.cosine_similarity_bytea(raw, x[r]))
            c = [np.float64(oracle.cosine_similarity_bytea(x[r], x[w])) for w in (w1, w2, w3)]
            exp = (((c[2] + 1) / 2) * ((c[1] + 1.0) / 2.0)) / (((c[0] + 1.0) / 2.0) + 0.001)   # freddy--0.0.1.sql:1243, in float8
            assert np.float64(mul[r]).view(np.uint64) == np.float64(exp).view(np.uint64), (w1, w2, w3, r)


def test_model_ordering_and_exclusion():
    ids = np.array([10, 20, 30, 40, 50, 60], np.int32)
    score = np.array([0.5, 0.9, 0.9, 0.1, 0.9, -0.0])
    i, s = am.topk(score, ids, {1}, 4)
    assert i.tolist() == [30, 50, 10, 40] and s.tolist() == [0.9, 0.9, 0.5, 0.1]
    nan = np.array([0.5, np.nan, 0.9, -np.nan, np.inf, 0.1])
    i, s = am.topk(nan, ids, {5}, 5)                 # NaN sorts first (PostgreSQL's float8 order), among equals by id
    assert i.tolist() == [20, 40, 50, 30, 10]
    assert s[:2].view(np.uint64).tolist() == [0x7ff8000000000000] * 2 and s[2:].tolist() == [np.inf, 0.9, 0.5]
    i, s = am.topk(score, ids, {0, 1, 2}, 5, rows=[0, 1, 2, 5])
    assert i.tolist() == [60, -1, -1, -1, -1] and np.signbit(s[0]) == False and np.isneginf(s[1:]).all()   # noqa: E712


# ---- codegen guard -------------------------------------------------------------------------------------------------------
PROBES = {
    "an_filter_kernel<3,false>": ("an_filter_kernel<3, false>", "an_filter_kernelILi3ELb0EE"),
    "an_filter_kernel<1,false>": ("an_filter_kernel<1, false>", "an_filter_kernelILi1ELb0EE"),
    "an_filter_kernel<3,true>": ("an_filter_kernel<3, true>", "an_filter_kernelILi3ELb1EE"),
    "an_scan_kernel<3,4>": ("an_scan_kernel<3, 4>", "an_scan_kernelILi3ELi4EE"),
    "an_scan_kernel<1,8>": ("an_scan_kernel<1, 8>", "an_scan_kernelILi1ELi8EE"),
    "an_refine_kernel<3>": ("an_refine_kernel<3>", "an_refine_kernelILi3EE"),
    "an_refine_kernel<1>": ("an_refine_kernel<1>", "an_refine_kernelILi1EE"),
    "an_filter_kernel<1,true>": ("an_filter_kernel<1, true>", "an_filter_kernelILi1ELb1EE"),
    "an_merge_kernel": ("an_merge_kernel", "15an_merge_kernelE"),
    "an_threshold_kernel": ("an_threshold_kernel", "19an_threshold_kernelE"),
    "an_gather_kernel": ("an_gather_kernel", "16an_gather_kernelE"),
}
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "an_probe.hip")
    with open(src, "w") as f:
        f.write('#include "analogy.h"\nusing namespace freddy;\nconst void* probe_kernels[] = {'
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
def test_analogy_kernels_do_not_spill(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill") if g[k]]
    for name, g in got.items():
        for k in ("vgprs", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            if g[k] > ceilings[name][k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {ceilings[name][k]}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_analogy_cpu.py [--write]: print (and commit) today's figures
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
