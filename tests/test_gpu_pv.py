"""-m gpu: batched post verification on the device (pv.h; freddy_gpu_ivfadc_search_pv, freddy_gpu_pq_search_pv,
freddy_gpu_last_pv_stats; the host mirror's k_nearest_neighbour_*_pv_batch and knn_batch()).  Expected lists come from the oracle
alone (tests/pv_model.py: approximate search at k * pvf -> drop ids < 0 and ids without a vector -> exact_knn over the rest); a
sample of queries is also compared with VectorIndex.search(q, k, subset_ids=candidates), the call the contract is written against.
The ANN handle's profile names the kernels that ran: stage one must be the plain search's own kernels, stage two pv_rerank."""
import numpy as np
import pytest

import mutation_model as mm
import pv_model as pm
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND = "freddy_gpu error -1", "freddy_gpu error -4"
CASES = [(5, 1), (5, 6), (5, 20), (1, 32), (30, 20), (64, 64)]   # no re-rank gain, fast scan, generic scan, fast scan, k > 512 passes, the limit


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _ivf_args(t):
    return t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"]


def _same_as_search(vec, qs, k, lists, gi, gs, sample, what):
    for qi in sample:
        cand = lists[qi][lists[qi] >= 0]
        si, ss = vec.search(qs[qi], k, subset_ids=cand if cand.size else np.array([-1], np.int32))
        assert np.array_equal(gi[qi], si[0]) and np.array_equal(gs[qi].view(np.uint32), ss[0].view(np.uint32)), (what, qi)


@pytest.fixture(scope="module")
def main(gpu, oracle):
    x, ids, qs, ivf, pq = pm.main_tables()
    h = {"x": x, "ids": ids, "qs": qs,
         "ivf": gpu.IVFIndex(*_ivf_args(ivf)), "pq": gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"]), "vec": gpu.VectorIndex(ids, x),
         "ivf_t": oracle.ivf_table(*_ivf_args(ivf)), "pq_t": oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])}
    yield h
    for n in ("ivf", "pq", "vec"):
        h[n].close()


@pytest.mark.parametrize("k,pvf", CASES)
def test_main_case(main, oracle, k, pvf):
    x, ids, qs, ivf, vec = main["x"], main["ids"], main["qs"], main["ivf"], main["vec"]
    kc, W = k * pvf, 3
    lists = pm.ivf_lists(oracle, main["ivf_t"], qs, kc, W)
    exp, n_cand, n_scored = pm.expected(oracle, lists, x, ids, qs, k)
    assert any((np.diff(e["dist"]) == 0).any() for e in exp[:20]) or k == 1, "no tie among the duplicate rows' queries"
    assert exp[6]["dist"][0] > 0.999                                          # (the query that is a table row finds it)
    for Q in (1, 70, 200):
        what = f"k={k} pvf={pvf} Q={Q}"
        _, plain = _profiled(ivf, lambda: ivf.search(qs[:Q], kc, W))
        (gi, gs), names = _profiled(ivf, lambda: ivf.search_pv(vec, qs[:Q], k, pvf, W))
        pm.same(gi, gs, exp[:Q], k, what)
        assert names == plain | {"pv_rerank"}, (what, sorted(names), sorted(plain))
        if Q >= 70:
            if kc > 512:
                assert {"merge_select", "bigk_replay", "adc_scan", "lut_build"} <= names, (what, sorted(names))
            elif kc > 32:
                assert {"lut_build", "adc_scan"} <= names and "ivf_filter" not in names, (what, sorted(names))
        assert ivf.last_pv_stats() == {"candidates": int(n_cand[:Q].sum()), "scored": int(n_scored[:Q].sum())}, what
        _same_as_search(vec, qs, k, lists, gi, gs, [q for q in (0, 3, 6, 12, 69, 199) if q < Q], what)


@pytest.mark.parametrize("k,pvf", [(5, 6), (5, 20), (30, 20)])
def test_pq(main, oracle, k, pvf):
    x, ids, qs, pq, vec = main["x"], main["ids"], main["qs"], main["pq"], main["vec"]
    kc, Q = k * pvf, 70 if k == 5 else 9
    rng = np.random.default_rng(3)
    rows = rng.choice(20000, 6000, replace=False)
    rows = np.union1d(rows, np.concatenate([np.arange(100, 140), np.arange(10000, 10040)]))
    subset = rng.permutation(np.concatenate([ids[rows], ids[rows[:50]], np.array([-5, 0, 10**8], np.int32)])).astype(np.int32)
    for sub, sentinel in ((None, 100.0), (subset, 1000.0)):
        lists = pm.pq_lists(oracle, main["pq_t"], qs[:Q], kc, sub)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x, ids, qs[:Q], k)
        for n in (1, Q):
            what = f"pq k={k} pvf={pvf} Q={n} subset={sub is not None}"
            _, plain = _profiled(pq, lambda: pq.search(qs[:n], kc, sentinel=sentinel, subset_ids=sub))
            (gi, gs), names = _profiled(pq, lambda: pq.search_pv(vec, qs[:n], k, pvf, sentinel=sentinel, subset_ids=sub))
            pm.same(gi, gs, exp[:n], k, what)
            assert names == plain | {"pv_rerank"}, (what, sorted(names), sorted(plain))
            assert pq.last_pv_stats() == {"candidates": int(n_cand[:n].sum()), "scored": int(n_scored[:n].sum())}, what
            _same_as_search(vec, qs, k, lists, gi, gs, [q for q in (0, 3, 6, 12) if q < n], what)


def test_missing_vectors(gpu, main, oracle):
    """The vector handle holds every second id: those candidates are dropped, scored < candidates."""
    x, ids, qs, ivf = main["x"], main["ids"], main["qs"][:70], main["ivf"]
    half = gpu.VectorIndex(ids[::2], x[::2])
    for k, pvf in ((5, 6), (5, 20)):
        lists = pm.ivf_lists(oracle, main["ivf_t"], qs, k * pvf, 3)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x[::2], ids[::2], qs, k)
        gi, gs = ivf.search_pv(half, qs, k, pvf, 3)
        pm.same(gi, gs, exp, k, f"every second vector, pvf={pvf}")
        st = ivf.last_pv_stats()
        assert st == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())} and 0 < st["scored"] < st["candidates"]
    half.close()


def test_fewer_candidates_than_k(gpu, oracle):
    """An index of 50 rows at k * pvf = 100: the lists end in fillers, the result rows in (-1, -inf); a vector handle that lacks
    some ids shortens them further; with W = 1 and a vector handle holding one cell's rows only, the queries of the other cell
    have no candidate with a vector: an empty row, not a search of the table."""
    import torch
    from freddy_amd import index_build as ib
    N, d = 50, 300
    x = util.corpus(20000).numpy()[:N].copy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    t = ib.build_ivf_index(torch.from_numpy(x), C=2, m=12, K=16, train_size=N, iters=3, seed=1)
    ivf, ot = gpu.IVFIndex(*_ivf_args(t)), oracle.ivf_table(*_ivf_args(t))
    qs = x[:20].copy()
    some = np.sort(np.random.default_rng(1).choice(N, 30, replace=False))
    for rows, what in ((np.arange(N), "all vectors"), (some, "30 vectors")):
        vec = gpu.VectorIndex(ids[rows], x[rows])
        lists = pm.ivf_lists(oracle, ot, qs, 100, 1)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x[rows], ids[rows], qs, 50)
        assert int(n_cand.sum()) == 20 * N and all(len(e) == rows.size for e in exp)
        gi, gs = ivf.search_pv(vec, qs, 50, 2, 1)
        pm.same(gi, gs, exp, 50, what)
        assert (gs[:, :rows.size] < 0).any() and (gs[:, 0] > 0).all()            # (negative similarities are ordered below the others)
        assert ivf.last_pv_stats() == {"candidates": 20 * N, "scored": 20 * int(rows.size)}
        vec.close()
    cell0 = np.sort(t["ids"][t["list_off"][0]:t["list_off"][1]])
    assert 2 <= cell0.size <= N - 2
    vec = gpu.VectorIndex(cell0, x[cell0 - 1])
    lists = pm.ivf_lists(oracle, ot, qs, 2, 1)
    exp, n_cand, n_scored = pm.expected(oracle, lists, x[cell0 - 1], cell0, qs, 2)
    empty = [len(e) == 0 for e in exp]
    assert any(empty) and not all(empty)
    gi, gs = ivf.search_pv(vec, qs, 2, 1, 1)
    pm.same(gi, gs, exp, 2, "one cell's vectors")
    assert ivf.last_pv_stats() == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())}
    gi, gs = ivf.search_pv(vec, np.empty((0, d), np.float32), 2, 1, 1)        # Q = 0
    assert gi.shape == (0, 2) and ivf.last_pv_stats() == {"candidates": 0, "scored": 0}
    vec.close()
    ivf.close()


@pytest.mark.parametrize("d,m,K", [(30, 5, 16), (25, 5, 16)])
def test_other_shapes(gpu, oracle, d, m, K):
    """d = 30 (rows of 120 bytes: a last step of 30 dimensions) and d = 25 (not a multiple of 4: rows not 16-byte aligned, the scalar loads)."""
    N, C = 6000, 16
    x = util.shape_corpus(N, d).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    qs = util.shape_queries(N, d, 70)
    qs[2] = -qs[2]
    it, pt = util.shape_ivf_tables(d, m, K, C, N), util.shape_pq_tables(d, m, K, N)
    ivf, pq, vec = gpu.IVFIndex(*_ivf_args(it)), gpu.PQIndex(pt["codebook"], pt["ids"], pt["codes"]), gpu.VectorIndex(ids, x)
    for k, pvf in ((5, 6), (5, 20), (3, 200)):
        lists = pm.ivf_lists(oracle, oracle.ivf_table(*_ivf_args(it)), qs, k * pvf, 3)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x, ids, qs, k)
        (gi, gs), names = _profiled(ivf, lambda: ivf.search_pv(vec, qs, k, pvf, 3))
        pm.same(gi, gs, exp, k, f"ivf d={d} k={k} pvf={pvf}")
        assert "pv_rerank" in names and ivf.last_pv_stats()["scored"] == int(n_scored.sum())
        _same_as_search(vec, qs, k, lists, gi, gs, (0, 2, 69), f"ivf d={d}")
        lists = pm.pq_lists(oracle, oracle.pq_table(pt["codebook"], pt["ids"], pt["codes"]), qs[:20], k * pvf)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x, ids, qs[:20], k)
        gi, gs = pq.search_pv(vec, qs[:20], k, pvf)
        pm.same(gi, gs, exp, k, f"pq d={d} k={k} pvf={pvf}")
    for h in (ivf, pq, vec):
        h.close()


@pytest.mark.parametrize("d,m,K", [(7, 1, 16), (32, 4, 16), (33, 3, 16)])
def test_small_tables_at_the_edges_of_a_step(gpu, oracle, d, m, K):
    """The re-rank's tile takes 32 dimensions per step: d = 7 (less than one step, odd: the scalar loads), 32 (one full step and no
    tail) and 33 (a tail of one dimension), over 300 rows and 40 queries, every third row without a vector; 1, 63, 64 candidates
    (one wave) and 65 (four waves)."""
    N = 300
    x = util.shape_corpus(N, d).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    qs = util.shape_queries(N, d, 40)
    pt = util.shape_pq_tables(d, m, K, N)
    keep = np.arange(N) % 3 != 0
    pq, vec = gpu.PQIndex(pt["codebook"], pt["ids"], pt["codes"]), gpu.VectorIndex(ids[keep], x[keep])
    pq_t = oracle.pq_table(pt["codebook"], pt["ids"], pt["codes"])
    for k, pvf in ((1, 1), (9, 7), (8, 8), (13, 5)):
        lists = pm.pq_lists(oracle, pq_t, qs, k * pvf)
        exp, n_cand, n_scored = pm.expected(oracle, lists, x[keep], ids[keep], qs, k)
        (gi, gs), names = _profiled(pq, lambda: pq.search_pv(vec, qs, k, pvf))
        pm.same(gi, gs, exp, k, f"pq d={d} k={k} pvf={pvf}")
        assert "pv_rerank" in names and pq.last_pv_stats()["scored"] == int(n_scored.sum())
    pq.close(); vec.close()


def test_after_append_rows(gpu, oracle):
    """Rows appended to the IVFADC handle AND to the vector handle: they must be found, resolved and able to win."""
    d, m, K, C, N, n0 = 30, 5, 16, 16, 6000, 5000
    t, x = util.shape_ivf_tables(d, m, K, C, N), util.shape_corpus(N, d).numpy()
    cell_sorted = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)
    cell, codes = np.empty(N, np.int32), np.empty((N, m), np.int16)
    cell[t["ids"] - 1] = cell_sorted
    codes[t["ids"] - 1] = t["codes"]
    ids = np.arange(1, N + 1, dtype=np.int32)
    model = mm.IVFModel.from_rows(t["coarse"], t["codebook"], ids[:n0], cell[:n0], codes[:n0])
    ivf, vec = gpu.IVFIndex(*model.pin_args()), gpu.VectorIndex(ids[:n0], x[:n0])
    qs = np.concatenate([x[n0:n0 + 40], x[:30]])
    n = n0
    for step in (37, 963):
        sl = slice(n, n + step)
        ivf.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]); model.append(ids[sl], cell[sl], codes[sl])
        vec.append_rows(ids[sl], vectors=x[sl])
        n += step
        for k, pvf in ((5, 6), (5, 20)):
            lists = pm.ivf_lists(oracle, model.oracle_table(oracle), qs, k * pvf, 3)
            exp, n_cand, n_scored = pm.expected(oracle, lists, x[:n], ids[:n], qs, k)
            gi, gs = ivf.search_pv(vec, qs, k, pvf, 3)
            pm.same(gi, gs, exp, k, f"after the append to {n} rows, pvf={pvf}")
            own = min(step, 40)   # the queries that are appended rows: each finds itself (or an older exact copy of itself, by id)
            assert (gi[:own, 0] > n0).sum() >= own - 4 and (gs[:own, 0] > 0.999).all(), "appended rows do not win their own queries"
            assert ivf.last_pv_stats() == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())}
    ivf.close()
    vec.close()


def test_refusals(gpu, main):
    qs, ivf, pq, vec = main["qs"][:4], main["ivf"], main["pq"], main["vec"]
    with pytest.raises(gpu.FreddyGpuError, match=E_KIND + ".*wrong kind"):
        pq.search_pv(ivf, qs, 5, 6)                                            # an ivf handle where the vectors belong
    oi, os_ = np.empty((4, 5), np.int32), np.empty((4, 5), np.float32)
    with pytest.raises(gpu.FreddyGpuError, match=E_KIND + ".*wrong kind"):     # swapped: vectors first
        gpu._check(ivf.lib.freddy_gpu_ivfadc_search_pv(vec.h, ivf.h, gpu._p(qs), 4, 5, 6, 3, gpu.C.c_float(1000.0), 0, gpu._p(oi), gpu._p(os_)))
    with pytest.raises(gpu.FreddyGpuError, match=E_KIND + ".*wrong kind"):     # a pq handle through the ivf entry point
        gpu._check(ivf.lib.freddy_gpu_ivfadc_search_pv(pq.h, vec.h, gpu._p(qs), 4, 5, 6, 3, gpu.C.c_float(1000.0), 0, gpu._p(oi), gpu._p(os_)))
    with pytest.raises(gpu.FreddyGpuError, match=E_KIND):
        gpu._check(ivf.lib.freddy_gpu_last_pv_stats(vec.h, None, None))
    other = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), util.shape_corpus(6000, 30).numpy()[:100])
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + ".*vectors have 30 dimensions, the index has 300"):
        ivf.search_pv(other, qs, 5, 6, 3)
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + ".*vectors have 30 dimensions, the index has 300"):
        pq.search_pv(other, qs, 5, 6)
    other.close()
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + ".*W must be positive"):
        ivf.search_pv(vec, qs, 5, 6, 0)
    t = pm.main_tables()[3]
    twice = gpu.IVFIndex(*_ivf_args(t), devices=[0, 0])
    assert twice.replicas == 2
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + ".*handle with replicas \\(2 devices\\)"):
        twice.search_pv(vec, qs, 5, 6, 3)
    twice.close()


# ---- the host mirror ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    from freddy_amd import udf
    N = 20000
    x = util.corpus(N).numpy()
    s = udf.Session()
    perm = np.random.default_rng(1).permutation(N)
    s.load_vecs_norm(np.arange(1, N + 1, dtype=np.int32)[perm], x[perm])
    pq, t = util.pq_tables(N=N, K=256), util.ivf_tables()
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    s.load_ivfadc(t["coarse"], t["codebook"], t["ids"], np.repeat(np.arange(32), np.diff(t["list_off"])).astype(np.int32), t["codes"])
    yield s, x
    s.close()


def test_host_mirror_batch_equals_the_single_query_functions(db):
    s, x = db
    rng = np.random.default_rng(9)
    qids = rng.choice(np.arange(1, 20001), 58, replace=False).astype(np.int32)
    qids = np.concatenate([qids, qids[:1], np.array([20000 + 7], np.int32)])            # 60 ids: a duplicate and an unknown one
    known = np.unique(qids[qids <= 20000])
    for pvf in (20, 6):
        s.set_pvf(pvf)
        for batch, single in ((s.k_nearest_neighbour_ivfadc_pv_batch, s.k_nearest_neighbour_ivfadc_pv),
                              (s.k_nearest_neighbour_pq_pv_batch, s.k_nearest_neighbour_pq_pv)):
            rows = batch(qids, 5)
            exp = [(int(q), int(r["id"]), r["distance"]) for q in known for r in single(x[q - 1], 5)]
            assert len(exp) == 5 * known.size
            assert rows["query_id"].tolist() == [e[0] for e in exp] and rows["id"].tolist() == [e[1] for e in exp]
            assert np.array_equal(rows["distance"].view(np.uint32), np.array([e[2] for e in exp], np.float32).view(np.uint32))
    s.set_pvf(1000)
    from freddy_amd import udf
    with pytest.raises(udf.FreddyError, match=r"^pvf \* k = 5000 exceeds this build's limit of 4096 candidates$"):
        s.k_nearest_neighbour_ivfadc_pv_batch(qids, 5)
    s.set_pvf(20)
    assert len(s.k_nearest_neighbour_pq_pv_batch([20000 + 7], 5)) == 0                  # no known query id: no rows


def test_knn_batch_dispatcher(db):
    from freddy_amd import udf
    s, x = db
    qids = np.array([11, 500, 7777, 42, 19999, 42], np.int32)
    assert s.get_knn_batch_function_name() == "k_nearest_neighbour_ivfadc_batch"
    plain = s.k_nearest_neighbour_ivfadc_batch(qids, 5)
    assert np.array_equal(s.knn_batch(qids, 5), plain)
    s.set_knn_batch_function("k_nearest_neighbour_ivfadc_pv_batch")
    pv = s.knn_batch(qids, 5)
    assert np.array_equal(pv, s.k_nearest_neighbour_ivfadc_pv_batch(qids, 5)) and not np.array_equal(pv, plain)
    s.set_knn_batch_function("k_nearest_neighbour_pq_pv_batch")
    assert np.array_equal(s.knn_batch(qids, 5), s.k_nearest_neighbour_pq_pv_batch(qids, 5))
    s.set_knn_batch_function("knn_batch_typo")
    with pytest.raises(udf.FreddyError, match=r"^function knn_batch_typo\(character varying\[\], integer\) does not exist$"):
        s.knn_batch(qids, 5)
    s.set_knn_batch_function("k_nearest_neighbour_ivfadc_batch")
