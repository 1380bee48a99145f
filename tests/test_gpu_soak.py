"""-m gpu: randomised soak of the IVFADC scans against the oracle with a FIXED seed budget (the long version
is tools/soak_fused.py): random shapes -- K from 4 to 1024, 1 to 40 cells incl. empty ones, 50 to 30 000
rows, 1 to 5000 distinct code rows (i.e. from "every distance equal" to "all different"), 1 to 700 queries
-- both cell-grouped scans and the generic kernels, both found rules.  Below them the fixed-seed forms of tools/soak_shapes.py,
tools/soak_bigk.py and the kNN-join part of tools/soak_round3.py: the draws are tests/soak_inputs.py's, which those tools loop over
too, and tests/test_soak_inputs_cpu.py proves which regimes the seed lists reach."""
import numpy as np
import pytest

import soak_inputs as si
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.mark.parametrize("seed", list(range(12)))
def test_soak_random_index(gpu, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    d, m = 300, 12
    K = int(rng.choice([4, 16, 64, 256, 1024]))
    C = int(rng.choice([1, 2, 5, 9, 40]))
    N = int(rng.choice([50, 700, 9000, 30000]))
    coarse = rng.standard_normal((C, d)).astype(np.float32)
    codebook = (rng.standard_normal((m, K, 25)) * 0.3).astype(np.float32)
    cell = rng.integers(0, C, size=N) if seed % 3 else np.zeros(N, np.int64)
    if C > 2:
        cell[cell == 1] = 0          # an empty list
    order = np.argsort(cell, kind="stable")
    ids = (np.arange(N) * 3 + 7).astype(np.int32)[order]
    n_distinct = int(rng.choice([1, 3, 50, 5000]))
    pool = rng.integers(0, K, size=(n_distinct, m)).astype(np.int16)
    codes = pool[rng.integers(0, n_distinct, size=N)][order]
    list_off = np.zeros(C + 1, np.int32)
    list_off[1:] = np.cumsum(np.bincount(cell, minlength=C))
    ids_sorted = np.concatenate([np.sort(ids[list_off[c]:list_off[c + 1]]) for c in range(C)]).astype(np.int32)
    ot = oracle.ivf_table(coarse, codebook, list_off, ids_sorted, codes)
    idx = gpu.IVFIndex(coarse, codebook, list_off, ids_sorted, codes)
    Q = int(rng.choice([1, 40, 300, 700]))
    qs = (coarse[rng.integers(0, C, size=Q)] + 0.2 * rng.standard_normal((Q, d))).astype(np.float32)
    for fused, variant in ((1, 5), (1, 3), (0, 5)):
        idx.set_option("fused", fused)
        idx.set_option("fused_kernel", variant)
        for k, W in [(1, 1), (5, min(3, C)), (32, min(C, 12))]:
            for rule, sent in [(0, 1000.0), (1, 100.0)]:
                gi, gd = idx.search(qs, k, W, sentinel=sent, found_rule=rule)
                exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
                util.assert_same_lists(gi, gd, exp, f"seed={seed} fused={fused} kernel={variant} K={K} C={C} N={N} Q={Q} "
                                                    f"k={k} W={W} rule={rule}")
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("seed", list(range(10)))
def test_soak_random_pq_table(gpu, oracle, seed):
    """Batches over random flat PQ tables (tools/soak_pq.py with a fixed seed budget): sizes around the pseudo-list
    boundaries, duplicate-heavy code pools, both paths, subsets."""
    rng = np.random.default_rng(5000 + seed)
    d, m = 300, 12
    K = int(rng.choice([16, 64, 256, 1024]))
    N = int(rng.choice([60, 4095, 4096, 4097, 9000, 40000, 70000]))
    codebook = (rng.standard_normal((m, K, 25)) * 0.3).astype(np.float32)
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    n_distinct = int(rng.choice([1, 7, 300, 100000]))
    pool = rng.integers(0, K, size=(n_distinct, m)).astype(np.int16)
    codes = pool[rng.integers(0, n_distinct, size=N)]
    ot = oracle.pq_table(codebook, ids, codes)
    idx = gpu.PQIndex(codebook, ids, codes)
    Q = int(rng.choice([16, 17, 48, 130]))
    qs = (0.5 * rng.standard_normal((Q, d))).astype(np.float32)
    if seed % 4 == 0:
        qs[0] *= np.float32(40.0)      # beyond the sentinel 100.0
    for k in (1, 5, 32):
        exp = np.stack([oracle.pq_search(ot, q, k) for q in qs])
        for mode in (1, 0):
            idx.set_option("pq_fused", mode)
            gi, gd = idx.search(qs, k, sentinel=100.0)
            util.assert_same_lists(gi, gd, exp, f"seed={seed} K={K} N={N} Q={Q} k={k} pq_fused={mode}")
    if N >= 9000:
        sub = rng.choice(ids, size=int(rng.choice([4200, 6000])), replace=False).astype(np.int32)
        sub = np.concatenate([sub, sub[:30], np.array([2, 4], np.int32)])
        exp = oracle.pq_search_in_batch(ot, qs, 5, sub, use_target_lists=True)
        for mode in (-1, 0):
            idx.set_option("pq_fused", mode)
            gi, gd = idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)
            util.assert_same_lists(gi, gd, exp, f"seed={seed} subset K={K} N={N} Q={Q} pq_fused={mode}")
    assert idx.bound_violations() == 0
    idx.close()


def run_shapes(gpu, d):
    """index shapes other than m = 12 / S = 25: multi.h's cell-grouped exact scan, the generic kernels, filter + refine with and
    without the running bound"""
    idx = gpu.IVFIndex(*d["pin"])
    for c in d["calls"]:
        for fused, rb in si.SHAPES_CONFIGS:
            idx.set_option("fused", fused)
            idx.set_option("running_bound", rb)
            gi, gd = idx.search(d["qs"], c["k"], c["W"], sentinel=c["sentinel"], found_rule=c["rule"])
            util.assert_same_lists(gi, gd, c["exp"], f"{d['label']} @ W={c['W']} k={c['k']} rule={c['rule']} fused={fused} rb={rb}")
    assert idx.bound_violations() == 0, d["label"]
    idx.close()


def run_bigk(gpu, d):
    """lists of 513 .. 4096 entries (bigk.h) from ivfadc_search, pq_search and pq_search_in, and the kNN-join's post verification
    of 1025 .. 8192 candidates, on tables with runs of equal distances"""
    idx = gpu.IVFIndex(*d["ivf_pin"])
    for c in d["ivf_calls"]:
        gi, gd = idx.search(d["qs"], c["k"], c["W"], sentinel=c["sentinel"], found_rule=c["rule"])
        util.assert_same_lists(gi, gd, c["exp"], f"{d['label']} @ ivfadc k={c['k']} W={c['W']} rule={c['rule']} sent={c['sentinel']}")
    assert idx.bound_violations() == 0, d["label"]
    idx.close()
    pidx = gpu.PQIndex(*d["pq_pin"])
    gi, gd = pidx.search(d["qs"], d["pq_k"], sentinel=100.0)
    util.assert_same_lists(gi, gd, d["pq_exp"], f"{d['label']} @ pq_search")
    gi, gd = pidx.search(d["qs"], d["pq_k"], sentinel=1000.0, subset_ids=d["pq_targets"])
    util.assert_same_lists(gi, gd, d["pq_in_exp"], f"{d['label']} @ pq_search_in")
    assert pidx.bound_violations() == 0, d["label"]
    pidx.close()
    if d["join"]:
        j = d["join"]
        jidx = gpu.IVPQIndex(*j["pin"])
        for c in j["calls"]:
            gi, gd, git = jidx.knn_join(j["qs"], c["k"], j["targets"], c["alpha"], c["pvf"], 2, use_target_lists=c["tl"], confidence=0.8)
            what = f"{d['label']} @ join k={c['k']} pvf={c['pvf']} alpha={c['alpha']} tl={c['tl']}"
            assert git == c["iterations"], (what, git, c["iterations"])
            util.assert_same_lists(gi, gd, c["exp"], what)
        jidx.close()


def run_join(gpu, d):
    """the kNN-join with the traversal on the device and on the host heap"""
    jdx = gpu.IVPQIndex(*d["pin"])
    for c in d["calls"]:
        for host in (0, 1):
            jdx.set_option("join_host_traversal", host)
            gi, gd, git = jdx.knn_join(d["qs"], c["k"], d["targets"], c["alpha"], c["pvf"], c["method"], use_target_lists=c["tl"], confidence=c["confidence"])
            what = f"{d['label']} @ k={c['k']} alpha={c['alpha']} pvf={c['pvf']} method={c['method']} conf={c['confidence']} tl={c['tl']} host={host}"
            assert git == c["iterations"], (what, git, c["iterations"])
            util.assert_same_lists(gi, gd, c["exp"], what)
    jdx.close()


@pytest.mark.parametrize("seed", si.SEEDS["shapes"])
def test_soak_shapes(gpu, oracle, seed):
    run_shapes(gpu, si.draw_shapes(seed, oracle))


@pytest.mark.parametrize("seed", si.SEEDS["bigk"])
def test_soak_bigk(gpu, oracle, seed):
    run_bigk(gpu, si.draw_bigk(seed, oracle))


@pytest.mark.parametrize("seed", si.SEEDS["join"])
def test_soak_join(gpu, oracle, seed):
    run_join(gpu, si.draw_join(seed, oracle))
