"""CPU suite for analogy_pair_direction (analogy.h, method FREDDY_ANALOGY_PAIR_DIRECTION of freddy_gpu_exact_analogy, the host
mirror's freddy_load_vecs_original / analogy_pair_direction): exported symbols, argument / limit errors without a GPU, the numpy
model (tests/pair_model.py) against the oracle's cosine_similarity_bytea / vec_normalize / vec_minus, and a codegen guard for the
two new kernels (0 VGPR spills, 0 scratch; VGPRs and SGPR spills within the committed ceilings)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pair_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
CEILINGS = os.path.join(ROOT, "tests", "golden", "pair_codegen_ceilings.json")
PAIR = 2   # include/freddy_gpu.h FREDDY_ANALOGY_PAIR_DIRECTION


def test_new_symbols_are_exported():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu, udf
    assert gpu.ANALOGY_METHODS["pair_direction"] == PAIR
    lib = udf.load()
    for n in ("freddy_load_vecs_original", "analogy_pair_direction"):
        assert hasattr(lib, n), n


def test_argument_and_limit_errors_without_a_gpu():
    from freddy_amd import gpu
    lib = gpu.load()
    t = np.array([[1, 2, 3]], np.int32)
    oi = np.empty(40, np.int32)
    os_ = np.empty(40, np.float64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    call = lambda ix, m, Q, k, sub=None, ns=0: lib.freddy_gpu_exact_analogy(ix, m, P(t), Q, k, sub, ns, P(oi), P(os_))   # noqa: E731
    assert call(None, PAIR, 1, 33) == -5 and b"33" in lib.freddy_gpu_last_error()       # FREDDY_E_LIMIT, k > 32
    assert call(None, PAIR, -1, 1) == -1 and call(None, PAIR, 1, 0) == -1               # bad sizes
    assert call(None, PAIR, 1, 1, None, 5) == -1                                        # a subset count without ids
    assert lib.freddy_gpu_exact_analogy(None, PAIR, None, 1, 1, None, 0, P(oi), P(os_)) == -1   # NULL triples
    assert b"NULL index" not in lib.freddy_gpu_last_error()
    assert call(None, PAIR, 1, 1) == -1 and b"NULL index" in lib.freddy_gpu_last_error()   # the method itself is accepted
    assert call(None, 3, 1, 1) == -1 and b"unknown analogy method" in lib.freddy_gpu_last_error()


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    with pytest.raises(udf.FreddyError, match=r"^google_vecs is not loaded$"):
        s.analogy_pair_direction(1, 2, 3)
    s.set_analogy_function("analogy_pair_direction")
    with pytest.raises(udf.FreddyError, match=r"^google_vecs is not loaded$"):          # dispatched, not "does not exist"
        s.analogy(1, 2, 3)
    s.set_analogy_in_function("analogy_pair_direction")                                 # the reference has no _in form
    with pytest.raises(udf.FreddyError, match=r"^function analogy_pair_direction\(unknown, unknown, unknown, character varying\[\]\) does not exist$"):
        s.analogy_in(1, 2, 3, [4, 5])
    s.close()


def test_model_equals_oracle_composition(oracle):
    """The model's float32 chains, square root and division equal the composition cosine_similarity_bytea(vec_normalize(vec_minus(v1,
    v2)), vec_normalize(vec_minus(v3, v4))) of the oracle bit for bit -- for every row, NaN scores included (compared as NaN)."""
    rng = np.random.default_rng(0)
    d, N = 300, 64
    x = rng.standard_normal((N, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    x[5] *= np.float32(3.5)                                        # not every row normalised
    x[40] = x[3]                                                   # a copy of (1, 2, 3)'s v3 under another row: length 0, NaN
    x[41] = (rng.standard_normal(d) * 1e-30).astype(np.float32)    # 1e-30-scale entries: their squares underflow to 0
    x[42] = (rng.standard_normal(d) * 1e-21).astype(np.float32)    # 1e-21-scale entries ...
    x[43] = x[42] * np.float32(1.5)                                # ... (5, 11, 42) against row 43: squares of 1e-43, denormal
    x_t = np.ascontiguousarray(x.T)
    triples = ((1, 2, 3), (7, 7, 9), (5, 11, 5), (5, 11, 42), (5, 11, 41))
    got = pm.scores(x, x_t, triples).astype(np.float32)
    for j, (w1, w2, w3) in enumerate(triples):
        a = oracle.vec_normalize(oracle.vec_minus(x[w1], x[w2]))
        exp = np.array([oracle.cosine_similarity_bytea(a, oracle.vec_normalize(oracle.vec_minus(x[w3], x[r]))) for r in range(N)], np.float32)
        assert np.array_equal(np.isnan(got[j]), np.isnan(exp)), (w1, w2, w3)
        ok = ~np.isnan(exp)
        assert np.array_equal(got[j][ok].view(np.uint32), exp[ok].view(np.uint32)), (w1, w2, w3, np.nonzero(got[j].view(np.uint32) != exp.view(np.uint32))[0][:5])
    assert np.isnan(got[1]).all(), "w1 == w2: A is 0/0 in every component, every score NaN"
    assert np.isnan(got[0][[3, 40]]).all() and np.isnan(got[0]).sum() == 2, "v3's own row and its copy, no other"
    assert np.isnan(got[2][5]) and np.isfinite(np.delete(got[2], 5)).all()
    sq = np.float32(0)
    for v in (x[42] - x[43]):
        sq = sq + v * v
    assert 0 < sq < np.finfo(np.float32).tiny and np.isfinite(got[3][43]), "the denormal sum of squares is a length, not 0"
    # the order the contract pins: the copy of v3 (NaN) first, v3 itself excluded
    ids = np.arange(100, 100 + N, dtype=np.int32)
    i, s = pm.model(x, ids, ids[[1, 2, 3]][None], 3)
    assert i[0, 0] == ids[40] and np.isnan(s[0, 0]) and np.isfinite(s[0, 1:]).all() and s[0, 1] >= s[0, 2]
    i, s = pm.model(x, ids, ids[[7, 7, 9]][None], 3)
    assert i[0].tolist() == ids[[0, 1, 2]].tolist() and np.isnan(s).all()
    i, s = pm.model(x, ids, [[100, 101, 5]], 2)
    assert (i == -1).all() and np.isneginf(s).all()


# ---- codegen guard -------------------------------------------------------------------------------------------------------
PROBES = {
    "an_pair_scan_kernel<1>": ("an_pair_scan_kernel<1>", "an_pair_scan_kernelILi1EE"),
    "an_pair_scan_kernel<2>": ("an_pair_scan_kernel<2>", "an_pair_scan_kernelILi2EE"),
    "an_pair_scan_kernel<4>": ("an_pair_scan_kernel<4>", "an_pair_scan_kernelILi4EE"),
    "an_pair_scan_kernel<8>": ("an_pair_scan_kernel<8>", "an_pair_scan_kernelILi8EE"),
    "an_pair_columns_kernel": ("an_pair_columns_kernel", "22an_pair_columns_kernelE"),
}
FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "pair_probe.hip")
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
def test_pair_kernels_do_not_spill(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill") if g[k]]
    for name, g in got.items():
        for k in ("vgprs", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            if g[k] > ceilings[name][k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {ceilings[name][k]}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_pair_direction_cpu.py [--write]: print (and commit) today's figures
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
