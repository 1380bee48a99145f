"""CPU suite for the assignment step of cluster_exact / cluster_pq (csrc/assign.h; freddy_gpu_exact_assign / freddy_gpu_pq_assign;
include/freddy_similarity.h): the model of tests/assign_model.py against the list-based definition it replaces, the shared
similarity function against the snprintf / strtof original bit for bit (a C program, plain and under ASan + UBSan), every argument, limit and
sentinel error that needs no device, and a codegen guard for the assign_ kernels (0 spilled VGPRs, 0 scratch; VGPRs and SGPRs
within tests/golden/assign_codegen_ceilings.json).  Handles of the wrong kind cannot exist without a device: tests/test_gpu_assign.py."""
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
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "postgres-word2vec_amd", "csrc")
CEILINGS = os.path.join(ROOT, "tests", "golden", "assign_codegen_ceilings.json")


# ---- 1. the model against the list-based definition ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(oracle):
    import util
    from freddy_amd import index_build as ib
    N, d = 600, 24
    x = util.shape_corpus(N, d).numpy().copy()
    x[300:340] = x[20:60]                      # duplicated table rows (beside shape_corpus' own 1 %)
    ids = np.arange(1, N + 1, dtype=np.int32)
    pq = ib.build_pq_index(torch.from_numpy(x), m=4, K=16, train_size=N, iters=3, seed=2)
    rng = np.random.default_rng(5)
    tokens = np.sort(np.concatenate([rng.choice(np.setdiff1d(ids, np.concatenate([np.arange(20, 61), np.arange(300, 341)])), 50, replace=False), np.arange(21, 41), np.arange(301, 321)])).astype(np.int32)
    assert tokens.size == 90 and np.unique(tokens).size == 90
    return dict(x=x, ids=ids, pq=pq, pt=oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"]), tokens=tokens, rng=rng)


def _centroids(t, kc, twin):
    """kc means of ten rows each (not rows); twin: the last one repeats the first."""
    rng = np.random.default_rng(100 + kc)
    c = np.stack([t["x"][rng.choice(600, 10)].mean(axis=0) for _ in range(kc)]).astype(np.float32)
    if twin and kc > 1:
        c[-1] = c[0]
    return c


@pytest.mark.parametrize("kc,twin", [(1, False), (5, False), (5, True), (17, True)])
def test_model_equals_the_first_row_per_token_of_the_lists(small, oracle, kc, twin):
    import assign_model as am
    from test_gpu_udf import _sim_of
    t = small
    tokens, n = t["tokens"], t["tokens"].size
    cent = _centroids(t, kc, twin)
    # exact: rows of knn_search_in_batch at k = n
    rows = []
    for qi, c in enumerate(cent):
        e = oracle.exact_knn(t["x"], t["ids"], c, n, tokens)
        assert len(e) == n
        rows += [(np.float32(e["dist"][r]), qi + 1, int(np.searchsorted(tokens, e["id"][r])) + 1) for r in range(n)]
    exp = am.first_per_token(rows, n)
    got = am.exact_assign(t["ids"], t["x"], cent, tokens)
    assert am.same(got, exp)
    assert (got[0] >= 0).all()
    if twin and kc > 1:
        assert not (got[0] == kc - 1).any(), "the copy of centroid 0 won a token: the lower index must"
    # duplicated rows get one answer
    a, b = np.searchsorted(tokens, np.arange(21, 41)), np.searchsorted(tokens, np.arange(301, 321))
    assert np.array_equal(got[0][a], got[0][b]) and np.array_equal(got[1][a].view(np.uint32), got[1][b].view(np.uint32))
    # pq: rows of pq_search_in_batch at k = n, similarity through the text round trip
    e = oracle.pq_search_in_batch(t["pt"], cent, n, tokens)
    rows = [(_sim_of(oracle, e["dist"][qi, r]), qi + 1, int(np.searchsorted(tokens, e["id"][qi, r])) + 1)
            for qi in range(kc) for r in range(n) if e["id"][qi, r] >= 0]
    exp = am.first_per_token(rows, n)
    got = am.pq_assign(oracle, t["pq"]["codebook"], t["pq"]["ids"], t["pq"]["codes"], cent, tokens, sentinel=1000.0)
    assert am.same(got, exp)
    assert (got[0] >= 0).all()


def test_model_positions_duplicates_and_unknown_ids(small, oracle):
    """A self-test of the numpy model alone (it runs no code of the project): positional outputs, duplicated and unknown ids, the
    strict sentinel and PostgreSQL's NaN order, which the device tests then take from the model."""
    import assign_model as am
    t = small
    cent = _centroids(t, 5, False)
    targets = np.array([40, 7, 40, 100000, -3, 7, 600, 1], np.int32)
    for got in (am.exact_assign(t["ids"], t["x"], cent, targets),
                am.pq_assign(oracle, t["pq"]["codebook"], t["pq"]["ids"], t["pq"]["codes"], cent, targets)):
        q, s = got
        assert q[3] == -1 and q[4] == -1 and np.isneginf(s[3]) and np.isneginf(s[4])
        assert q[0] == q[2] and q[1] == q[5] and s[0] == s[2] and s[1] == s[5]
        assert (np.delete(q, [3, 4]) >= 0).all()
    # a sentinel no distance is below: nothing is a candidate
    q, s = am.pq_assign(oracle, t["pq"]["codebook"], t["pq"]["ids"], t["pq"]["codes"], cent, targets, sentinel=0.0)
    assert (q == -1).all() and np.isneginf(s).all()
    # PostgreSQL's order: a NaN similarity wins, the first of two NaNs wins
    cent2 = cent.copy(); cent2[2, 3] = np.nan; cent2[4, 0] = np.nan
    q, s = am.exact_assign(t["ids"], t["x"], cent2, targets[:3])
    assert (q == 2).all() and np.isnan(s).all()


# ---- 2. the shared similarity function -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "asan_ubsan"])
def test_shared_similarity_equals_the_text_round_trip(kind, tmp_path):
    """Every binary32 of 2^22 consecutive values around 0.5, 1, 2 and 4, every exact .5 tie of dist * 1e6 below 16, 10^6 random
    values in [0, 1000), the values just below 1000, just above 0 and just below 2^24 (the end of the function's domain): the emitted
    distance and the similarity agree bit for bit.  tests/assign_sim_check.c is a program of its own: built plain, and built with
    ASan + UBSan (their runtimes linked into it) and run as it is."""
    exe = str(tmp_path / ("assign_sim_check_" + kind))
    flags = ["-O2"]
    if kind == "asan_ubsan":
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan"]
    subprocess.check_call(["gcc"] + flags + ["-std=c11", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-o", exe,
                                             "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "assign_sim_check.c"), "-lm"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    assert p.returncode == 0, "freddy_similarity.h differs from snprintf / strtof (mismatches, first bits, section):\n" + p.stdout[-2000:] + p.stderr[-3000:]
    assert len(lines) == 9 and all(ln.startswith("0 ") for ln in lines), p.stdout


# ---- 3. declarations, argument / limit / sentinel errors -------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from freddy_amd import gpu, udf
    decl = lambda h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)   # noqa: E731
    gh, uh = decl("freddy_gpu.h"), decl("freddy_udf.h")
    for n in ("freddy_gpu_exact_assign", "freddy_gpu_pq_assign"):
        assert re.search(r"\b" + n + r"\s*\(", gh) and hasattr(gpu.load(), n) and n in gpu.EXPORTS, n
    for n in ("exact_assign", "pq_assign"):
        assert re.search(r"\b" + n + r"\s*\(", uh) and hasattr(udf.load(), n), n
    assert hasattr(gpu.VectorIndex, "assign") and hasattr(gpu.PQIndex, "assign")
    assert hasattr(udf.Session, "exact_assign") and hasattr(udf.Session, "pq_assign")


def test_argument_limit_and_sentinel_errors_without_a_gpu():
    """Sizes, NULL buffers, the sentinel's range and the query limit are reported before the handle is looked at: FREDDY_E_ARG = -1,
    FREDDY_E_LIMIT = -5, each with the offending value in the message; then the NULL handle."""
    from freddy_amd import gpu
    lib = gpu.load()
    q = np.zeros((2, 8), np.float32)
    t = np.array([1, 2, 3], np.int32)
    oq, os_ = np.empty(3, np.int32), np.empty(3, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    err = lib.freddy_gpu_last_error
    f = ctypes.c_float

    def exact(Q, n, qp=P(q), tp=P(t), op=P(oq), sp=P(os_)):
        return lib.freddy_gpu_exact_assign(None, qp, Q, tp, n, op, sp)

    def pq(Q, n, qp=P(q), tp=P(t), op=P(oq), sp=P(os_), sentinel=1000.0):
        return lib.freddy_gpu_pq_assign(None, qp, Q, f(sentinel), tp, n, op, sp)

    for call in (exact, pq):
        assert call(-1, 3) == -1 and b"bad sizes" in err() and b"Q=-1" in err()
        assert call(2, -5) == -1 and b"bad sizes" in err() and b"n_targets=-5" in err()
        for hole in ("qp", "tp", "op", "sp"):
            assert call(2, 3, **{hole: None}) == -1 and b"NULL buffer" in err(), hole
        assert call(65537, 3) == -5 and b"Q=65537 exceeds this build's limit of 65536 queries" in err()
        assert call(2**31 - 1, 3) == -5 and b"Q=2147483647 " in err()
        assert call(65536, 3) == -1 and b"NULL index" in err()                                  # the limit itself is accepted
        assert call(2, 3) == -1 and b"NULL index" in err()
        assert call(0, 3, qp=None, tp=None, op=None, sp=None) == -1 and b"NULL index" in err()   # no work needs no buffers, but a handle
        assert call(2, 0, qp=None, tp=None, op=None, sp=None) == -1 and b"NULL index" in err()
        assert call(2, 2**40, tp=None) == -1 and b"NULL buffer" in err()                        # (a 64-bit count)
    assert pq(2, 3, sentinel=16777216.0) == -1 and b"NULL index" in err()                        # 2^24 itself is accepted
    assert pq(2, 3, sentinel=-1.0) == -1 and b"NULL index" in err()
    assert pq(2, 3, sentinel=16777218.0) == -1 and b"sentinel=1.67772e+07" in err() and b"2^24" in err()
    assert pq(2, 3, sentinel=float("inf")) == -1 and b"sentinel=inf" in err()
    assert pq(2, 3, sentinel=float("nan")) == -1 and b"sentinel=" in err() and b"2^24" in err()


def test_host_mirror_errors_without_a_gpu():
    from freddy_amd import udf
    s = udf.Session()
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
        s.exact_assign(q, [1, 2])
    with pytest.raises(udf.FreddyError, match="pq_quantization / pq_codebook are not loaded"):
        s.pq_assign(q, [1, 2])
    with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
        s.cluster_exact(np.arange(1, 5001, dtype=np.int32), 7)
    s.close()


# ---- 4. codegen guard --------------------------------------------------------------------------------------------------------
PROBES = {
    "assign_exact_kernel": ("assign_exact_kernel", "assign_exact_kernelENS_15AssignExactArgsE"),
    "assign_pq_kernel<6, 1>": ("assign_pq_kernel<6, 1>", "assign_pq_kernelILi6ELi1EE"),
    "assign_pq_kernel<6, 4>": ("assign_pq_kernel<6, 4>", "assign_pq_kernelILi6ELi4EE"),
    "assign_pq_kernel<0, 1>": ("assign_pq_kernel<0, 1>", "assign_pq_kernelILi0ELi1EE"),
    "assign_pq_kernel<0, 4>": ("assign_pq_kernel<0, 4>", "assign_pq_kernelILi0ELi4EE"),
}
FIELDS = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}


def measure(tmp):
    import __graft_entry__ as g
    flags = [f for f in g.HIPCC_FLAGS if f != "-fPIC"]
    src = os.path.join(tmp, "assign_probe.hip")
    with open(src, "w") as f:
        f.write('#include "assign.h"\nusing namespace freddy;\nconst void* probe_kernels[] = {'
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
def test_assign_kernels_do_not_spill(tmp_path):
    ceilings = json.load(open(CEILINGS))
    got = measure(str(tmp_path))
    bad = [f"{name}: {k} = {g[k]}, must be 0" for name, g in got.items() for k in ("scratch_bytes", "vgpr_spill") if g[k]]
    for name, g in got.items():
        for k in ("vgprs", "sgprs", "scratch_bytes", "vgpr_spill", "sgpr_spill"):
            if g[k] > ceilings[name][k]:
                bad.append(f"{name}: {k} = {g[k]} > ceiling {ceilings[name][k]}")
    assert not bad, "\n".join(bad) + "\n(measured: " + json.dumps(got) + ")"


if __name__ == "__main__":   # python tests/test_assign_cpu.py [--write]: print (and commit) today's figures
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        res = measure(td)
    print(json.dumps(res, indent=1))
    if "--write" in sys.argv:
        with open(CEILINGS, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
