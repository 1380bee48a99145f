"""-m gpu: batched approximate analogies on the device (approx_analogy.h; freddy_gpu_ivfadc_analogy, freddy_gpu_pq_analogy,
freddy_gpu_last_approx_analogy_stats; the host mirror's analogy_3cosadd_*_batch).  Expected rows come from the oracle alone
(tests/approx_analogy_model.py: vec_minus / vec_plus / vec_normalize -> approximate search at n_cand -> drop ids < 0, ids without a
vector and the inputs -> exact_knn of RAW over the rest); a sample of triples is also compared with VectorIndex.search(raw, k,
subset_ids=S), the call the contract is written against.  The ANN handle's profile names the kernels that ran: stage one must be the
plain search's own kernels, in front of it aa_query, behind it aa_rerank."""
import numpy as np
import pytest

import approx_analogy_model as am
import mutation_model as mm
import pv_model as pm
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND, E_LIMIT = "freddy_gpu error -1", "freddy_gpu error -4", "freddy_gpu error -5"
# one-wave re-rank; the reference's pvf = 20; the 64 / 65 boundary to the four-wave kernel; k > 512 passes of stage one; the limit
CASES = [(1, 4), (1, 23), (5, 64), (5, 65), (32, 640), (64, 4096)]
AA = {"aa_query", "aa_rerank"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    prof = idx.profile_read()
    idx.profile_enable(False)
    return out, prof


def _ivf_args(t):
    return t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"]


def _same_as_search(vec, vec_ids, triples, k, res, gi, gs, sample, what):
    """rows of the sample equal VectorIndex.search(raw, k, subset_ids=S)"""
    exp, st, lists, raw, valid = res
    pos = np.cumsum(valid) - 1
    for q in sample:
        if not valid[q]:
            continue
        _, have = pm.candidates(lists[pos[q]], vec_ids)
        S = have[~np.isin(have, triples[q])]
        si, ss = vec.search(raw[pos[q]], k, subset_ids=S if S.size else np.array([-1], np.int32))
        assert np.array_equal(gi[q], si[0]) and np.array_equal(gs[q].view(np.uint32), ss[0].view(np.uint32)), (what, q)


def _head(res, x, vec_ids, triples, k, Q, oracle):
    """the model for the first Q triples of a batch whose lists are known"""
    exp, st, lists, raw, valid = res
    n = int(valid[:Q].sum())
    return am.expected(oracle, lists[:n], valid[:Q], raw[:n], x, vec_ids, triples[:Q], k)


@pytest.fixture(scope="module")
def main(gpu, oracle):
    x, ids, qs, ivf, pq = pm.main_tables()
    h = {"x": x, "ids": ids, "t": am.main_triples(),
         "ivf": gpu.IVFIndex(*_ivf_args(ivf)), "pq": gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"]), "vec": gpu.VectorIndex(ids, x),
         "ivf_t": oracle.ivf_table(*_ivf_args(ivf)), "pq_t": oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])}
    yield h
    for n in ("ivf", "pq", "vec"):
        h[n].close()


@pytest.mark.parametrize("k,n_cand", CASES)
def test_main_case(main, oracle, k, n_cand):
    x, ids, t, ivf, vec = main["x"], main["ids"], main["t"], main["ivf"], main["vec"]
    W = 3
    res = am.ivf_expected(oracle, main["ivf_t"], x, ids, t, k, n_cand, W)
    exp, st, lists, raw, valid = res
    _, _, unit = am.build_queries(oracle, x, ids, t)
    assert valid.all() and st["scored"] < st["candidates"]          # (inputs were among the candidates: test_approx_analogy_cpu.py has the rest)
    for Q in (1, 70, 200):
        what = f"k={k} n_cand={n_cand} Q={Q}"
        _, plain = _profiled(ivf, lambda: ivf.search(unit[:Q], n_cand, W))
        (gi, gs), prof = _profiled(ivf, lambda: ivf.analogy(vec, t[:Q], k, n_cand, W))
        e, s = _head(res, x, ids, t, k, Q, oracle)
        pm.same(gi, gs, e, k, what)
        assert set(prof) == set(plain) | AA, (what, sorted(prof), sorted(plain))
        assert prof["aa_query"][0] == 1 and prof["aa_rerank"][0] == 1, what
        if Q >= 70 and n_cand > 512:
            assert {"merge_select", "bigk_replay"} <= set(prof), (what, sorted(prof))
        assert ivf.last_approx_analogy_stats() == s, what
        _same_as_search(vec, ids, t, k, res, gi, gs, [q for q in (0, 5, 60, 69, 100, 199) if q < Q], what)


@pytest.mark.parametrize("k,n_cand", [(1, 23), (5, 64)])
def test_pq(main, oracle, k, n_cand):
    x, ids, pq, vec = main["x"], main["ids"], main["pq"], main["vec"]
    t = main["t"][:70]
    rng = np.random.default_rng(3)
    keep = np.setdiff1d(ids, t[::2].ravel())                                      # the subset lacks the inputs of every second triple
    subset = rng.permutation(np.concatenate([rng.choice(keep, 797, replace=False), np.array([-5, 0, 10**8], np.int32)])).astype(np.int32)
    assert subset.size == 800
    _, _, unit = am.build_queries(oracle, x, ids, t)
    for sub, sentinel in ((None, 100.0), (subset, 1000.0)):
        res = am.pq_expected(oracle, main["pq_t"], x, ids, t, k, n_cand, sub)
        for n in (1, 70):
            what = f"pq k={k} n_cand={n_cand} Q={n} subset={sub is not None}"
            _, plain = _profiled(pq, lambda: pq.search(unit[:n], n_cand, sentinel=sentinel, subset_ids=sub))
            (gi, gs), prof = _profiled(pq, lambda: pq.analogy(vec, t[:n], k, n_cand, sentinel=sentinel, subset_ids=sub))
            e, s = _head(res, x, ids, t, k, n, oracle)
            pm.same(gi, gs, e, k, what)
            assert set(prof) == set(plain) | AA, (what, sorted(prof), sorted(plain))
            assert pq.last_approx_analogy_stats() == s, what
            _same_as_search(vec, ids, t, k, res, gi, gs, [q for q in (0, 5, 60) if q < n], what)


def test_unknown_ids(main, oracle):
    """A triple with an unknown id at the first, a middle and the last position: its row is (-1, -inf), its neighbours' rows are what
    they are without it, searched == Q - 3; a batch of unknown triples alone launches nothing."""
    x, ids, ivf, pq, vec = main["x"], main["ids"], main["ivf"], main["pq"], main["vec"]
    t = main["t"][:70].copy()
    clean_i, clean_s = ivf.analogy(vec, t, 5, 64, 3)
    t[0, 1], t[31, 0], t[69, 2] = 10**8, -7, 20001
    bad = np.array([0, 31, 69])
    exp, st, _, _, valid = am.ivf_expected(oracle, main["ivf_t"], x, ids, t, 5, 64, 3)
    assert (~valid).nonzero()[0].tolist() == bad.tolist() and st["searched"] == 67
    (gi, gs), prof = _profiled(ivf, lambda: ivf.analogy(vec, t, 5, 64, 3))
    pm.same(gi, gs, exp, 5, "unknown ids")
    assert (gi[bad] == -1).all() and np.isneginf(gs[bad]).all()
    ok = np.setdiff1d(np.arange(70), bad)
    assert np.array_equal(gi[ok], clean_i[ok]) and np.array_equal(gs[ok].view(np.uint32), clean_s[ok].view(np.uint32))
    assert ivf.last_approx_analogy_stats() == st and prof["aa_rerank"][0] == 1
    for idx, call in ((ivf, lambda: ivf.analogy(vec, t[bad], 5, 64, 3)), (pq, lambda: pq.analogy(vec, t[bad], 5, 64))):
        (gi, gs), prof = _profiled(idx, call)
        assert (gi == -1).all() and np.isneginf(gs).all() and gi.shape == (3, 5)
        assert prof == {}, sorted(prof)
        assert idx.last_approx_analogy_stats() == {"searched": 0, "candidates": 0, "scored": 0}
    gi, gs = ivf.analogy(vec, np.empty((0, 3), np.int32), 5, 64, 3)               # Q = 0
    assert gi.shape == (0, 5) and ivf.last_approx_analogy_stats() == {"searched": 0, "candidates": 0, "scored": 0}


def test_missing_vectors(gpu, main, oracle):
    """The vector handle lacks every fifth id: candidates without a row drop out, a triple whose input lacks a row is unknown."""
    x, ids, ivf, t = main["x"], main["ids"], main["ivf"], main["t"][:70]
    keep = ids % 5 != 0
    part = gpu.VectorIndex(ids[keep], x[keep])
    for k, n_cand in ((1, 23), (5, 65)):
        exp, st, _, _, valid = am.ivf_expected(oracle, main["ivf_t"], x[keep], ids[keep], t, k, n_cand, 3)
        assert 0 < st["searched"] < 70 and 0 < st["scored"] < st["candidates"]
        gi, gs = ivf.analogy(part, t, k, n_cand, 3)
        pm.same(gi, gs, exp, k, f"every fifth vector missing, n_cand={n_cand}")
        assert ivf.last_approx_analogy_stats() == st
    part.close()


def test_degenerate_query(gpu, oracle):
    """One all-zero row z: the triple (a, z, a) has raw = 0, length 0 and a unit row of NaN.  No special case: the model's row."""
    d, m, K, C, N = 30, 5, 16, 16, 6000
    x = util.shape_corpus(N, d).numpy().copy()
    x[1234] = 0.0
    ids = np.arange(1, N + 1, dtype=np.int32)
    it, pt = util.shape_ivf_tables(d, m, K, C, N), util.shape_pq_tables(d, m, K, N)
    ivf, pq, vec = gpu.IVFIndex(*_ivf_args(it)), gpu.PQIndex(pt["codebook"], pt["ids"], pt["codes"]), gpu.VectorIndex(ids, x)
    t = np.array([[10, 20, 30], [77, 1235, 77], [40, 50, 60], [1235, 1235, 1235]], np.int32)
    valid, raw, unit = am.build_queries(oracle, x, ids, t)
    assert valid.all() and not raw[1].any() and np.isnan(unit[1]).all() and np.isnan(unit[3]).all()
    for k, n_cand in ((1, 23), (5, 64), (5, 100)):
        exp, st, *_ = am.ivf_expected(oracle, oracle.ivf_table(*_ivf_args(it)), x, ids, t, k, n_cand, 3)
        gi, gs = ivf.analogy(vec, t, k, n_cand, 3)
        pm.same(gi, gs, exp, k, f"ivf raw = 0, n_cand={n_cand}")
        assert ivf.last_approx_analogy_stats() == st
        exp, st, *_ = am.pq_expected(oracle, oracle.pq_table(pt["codebook"], pt["ids"], pt["codes"]), x, ids, t, k, n_cand)
        gi, gs = pq.analogy(vec, t, k, n_cand)
        pm.same(gi, gs, exp, k, f"pq raw = 0, n_cand={n_cand}")
        assert pq.last_approx_analogy_stats() == st
    for h in (ivf, pq, vec):
        h.close()


@pytest.mark.parametrize("d,m,K", [(30, 5, 16), (25, 5, 16)])
def test_other_shapes(gpu, oracle, d, m, K):
    """d = 30 (rows of 120 bytes) and d = 25 (not a multiple of 4: rows not 16-byte aligned) through both kernels."""
    N, C = 6000, 16
    x = util.shape_corpus(N, d).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    t = np.random.default_rng(d).choice(ids, (70, 3)).astype(np.int32)
    t[3, 2] = t[3, 0]
    it, pt = util.shape_ivf_tables(d, m, K, C, N), util.shape_pq_tables(d, m, K, N)
    ivf, pq, vec = gpu.IVFIndex(*_ivf_args(it)), gpu.PQIndex(pt["codebook"], pt["ids"], pt["codes"]), gpu.VectorIndex(ids, x)
    for k, n_cand in ((1, 23), (5, 64), (3, 600)):
        res = am.ivf_expected(oracle, oracle.ivf_table(*_ivf_args(it)), x, ids, t, k, n_cand, 3)
        (gi, gs), prof = _profiled(ivf, lambda: ivf.analogy(vec, t, k, n_cand, 3))
        pm.same(gi, gs, res[0], k, f"ivf d={d} k={k} n_cand={n_cand}")
        assert AA <= set(prof) and ivf.last_approx_analogy_stats() == res[1]
        _same_as_search(vec, ids, t, k, res, gi, gs, (0, 3, 69), f"ivf d={d}")
        res = am.pq_expected(oracle, oracle.pq_table(pt["codebook"], pt["ids"], pt["codes"]), x, ids, t[:20], k, n_cand)
        gi, gs = pq.analogy(vec, t[:20], k, n_cand)
        pm.same(gi, gs, res[0], k, f"pq d={d} k={k} n_cand={n_cand}")
        assert pq.last_approx_analogy_stats() == res[1]
    for h in (ivf, pq, vec):
        h.close()


@pytest.mark.parametrize("d,m,K", [(7, 1, 16), (32, 4, 16), (33, 3, 16)])
def test_small_tables_at_the_edges_of_a_step(gpu, oracle, d, m, K):
    """The re-rank's tile takes 32 dimensions per step: d = 7 (less than one step, odd: the scalar loads), 32 (one full step and no
    tail) and 33 (a tail of one dimension), over 300 rows and 40 triples, every fifth row without a vector; 1 and 63 candidates
    (one wave), 65 (four waves)."""
    N = 300
    x = util.shape_corpus(N, d).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    t = np.random.default_rng(d).choice(ids, (40, 3)).astype(np.int32)
    pt = util.shape_pq_tables(d, m, K, N)
    keep = ids % 5 != 0
    pq, vec = gpu.PQIndex(pt["codebook"], pt["ids"], pt["codes"]), gpu.VectorIndex(ids[keep], x[keep])
    pq_t = oracle.pq_table(pt["codebook"], pt["ids"], pt["codes"])
    for k, n_cand in ((1, 1), (5, 63), (5, 65)):
        res = am.pq_expected(oracle, pq_t, x[keep], ids[keep], t, k, n_cand)
        gi, gs = pq.analogy(vec, t, k, n_cand)
        pm.same(gi, gs, res[0], k, f"pq d={d} k={k} n_cand={n_cand}")
        assert pq.last_approx_analogy_stats() == res[1]
    pq.close(); vec.close()


def test_pass_boundary(main, oracle):
    """analogy_pass = 64 with 130 triples and an unknown one at position 64: three passes, the rows and the stats of the default."""
    x, ids, ivf, vec = main["x"], main["ids"], main["ivf"], main["vec"]
    t = main["t"][:130].copy()
    t[64, 1] = 10**8
    exp, st, *_ = am.ivf_expected(oracle, main["ivf_t"], x, ids, t, 5, 64, 3)
    (di, ds), prof = _profiled(ivf, lambda: ivf.analogy(vec, t, 5, 64, 3))
    dst = ivf.last_approx_analogy_stats()
    assert prof["aa_rerank"][0] == 1
    ivf.set_option("analogy_pass", 64)
    try:
        (gi, gs), prof = _profiled(ivf, lambda: ivf.analogy(vec, t, 5, 64, 3))
        assert prof["aa_query"][0] == 3 and prof["aa_rerank"][0] == 3              # 129 triples: 64 + 64 + 1
        assert ivf.last_approx_analogy_stats() == dst == st
    finally:
        ivf.set_option("analogy_pass", 0)
    pm.same(gi, gs, exp, 5, "analogy_pass = 64")
    assert np.array_equal(gi, di) and np.array_equal(gs.view(np.uint32), ds.view(np.uint32))


def test_after_append_rows(gpu, oracle):
    """Rows appended to the IVFADC handle AND to the vector handle: a triple that names an appended id is answered, and appended
    rows are among the answers."""
    d, m, K, C, N, n0 = 30, 5, 16, 16, 6000, 5000
    t, x = util.shape_ivf_tables(d, m, K, C, N), util.shape_corpus(N, d).numpy()
    cell_sorted = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)
    cell, codes = np.empty(N, np.int32), np.empty((N, m), np.int16)
    cell[t["ids"] - 1] = cell_sorted
    codes[t["ids"] - 1] = t["codes"]
    ids = np.arange(1, N + 1, dtype=np.int32)
    model = mm.IVFModel.from_rows(t["coarse"], t["codebook"], ids[:n0], cell[:n0], codes[:n0])
    ivf, vec = gpu.IVFIndex(*model.pin_args()), gpu.VectorIndex(ids[:n0], x[:n0])
    rng = np.random.default_rng(8)
    tr = rng.choice(ids[:n0], (60, 3)).astype(np.int32)
    tr[:30, 1] = ids[n0:n0 + 30]                                                  # w2 an id that exists only after the first append
    tr[:30, 2] = tr[:30, 0]                                                       # ... and raw = its vector: its neighbours answer
    exp, st, *_ = am.ivf_expected(oracle, model.oracle_table(oracle), x[:n0], ids[:n0], tr, 5, 64, 3)
    assert st["searched"] == 30
    gi, gs = ivf.analogy(vec, tr, 5, 64, 3)
    pm.same(gi, gs, exp, 5, "before the append")
    n = n0
    for step in (37, 963):
        sl = slice(n, n + step)
        ivf.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]); model.append(ids[sl], cell[sl], codes[sl])
        vec.append_rows(ids[sl], vectors=x[sl])
        n += step
        for k, n_cand in ((1, 23), (5, 64)):
            exp, st, *_ = am.ivf_expected(oracle, model.oracle_table(oracle), x[:n], ids[:n], tr, k, n_cand, 3)
            assert st["searched"] == 60
            gi, gs = ivf.analogy(vec, tr, k, n_cand, 3)
            pm.same(gi, gs, exp, k, f"after the append to {n} rows, n_cand={n_cand}")
            assert ivf.last_approx_analogy_stats() == st
        assert (gi > n0).any(), "no appended row is ever an answer"
    ivf.close()
    vec.close()


def test_refusals(gpu, main):
    t, ivf, pq, vec = main["t"][:4], main["ivf"], main["pq"], main["vec"]
    C = gpu.C
    oi, os_ = np.empty((4, 5), np.int32), np.empty((4, 5), np.float32)
    sub = np.array([1, 2, 3], np.int32)

    def raw_ivf(a, v, Q=4, k=5, n_cand=64, W=3, rule=0, tp=gpu._p(t), ip=gpu._p(oi), sp=gpu._p(os_)):
        gpu._check(ivf.lib.freddy_gpu_ivfadc_analogy(a.h, v.h, tp, Q, k, n_cand, W, C.c_float(1000.0), rule, ip, sp))

    def raw_pq(a, v, Q=4, k=5, n_cand=64, subp=None, ns=0, tp=gpu._p(t), ip=gpu._p(oi), sp=gpu._p(os_)):
        gpu._check(pq.lib.freddy_gpu_pq_analogy(a.h, v.h, tp, Q, k, n_cand, C.c_float(100.0), subp, ns, ip, sp))

    other = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), util.shape_corpus(6000, 30).numpy()[:100])
    twice = gpu.IVFIndex(*_ivf_args(pm.main_tables()[3]), devices=[0, 0])
    assert twice.replicas == 2
    for idx in (ivf, pq, twice):
        idx.profile_enable(True)
    refused = [
        (lambda: raw_ivf(ivf, vec, Q=-1), E_ARG + ".*bad sizes.*Q=-1"),
        (lambda: raw_ivf(ivf, vec, k=0), E_ARG + ".*bad sizes.*k=0"),
        (lambda: raw_ivf(ivf, vec, k=5, n_cand=4), E_ARG + ".*bad sizes.*n_cand=4"),
        (lambda: raw_ivf(ivf, vec, W=0), E_ARG + ".*W must be positive"),
        (lambda: raw_ivf(ivf, vec, rule=3), E_ARG + ".*bad found_rule"),
        (lambda: raw_ivf(ivf, vec, rule=2), E_ARG + ".*FREDDY_FOUND_BATCH_UDF needs W == 1"),
        (lambda: raw_ivf(ivf, vec, tp=None), E_ARG + ".*NULL buffer"),
        (lambda: raw_ivf(ivf, vec, ip=None), E_ARG + ".*NULL buffer"),
        (lambda: raw_ivf(ivf, vec, sp=None), E_ARG + ".*NULL buffer"),
        (lambda: raw_ivf(ivf, vec, n_cand=4097), E_LIMIT + ".*n_cand = 4097 exceeds this build's limit of 4096 candidates"),
        (lambda: raw_ivf(vec, ivf), E_KIND + ".*wrong kind"),                      # swapped: vectors first
        (lambda: raw_ivf(pq, vec), E_KIND + ".*wrong kind"),                       # a pq handle through the ivf entry point
        (lambda: raw_ivf(ivf, pq), E_KIND + ".*wrong kind"),                       # a pq handle where the vectors belong
        (lambda: raw_ivf(ivf, other), E_ARG + ".*vectors have 30 dimensions, the index has 300"),
        (lambda: raw_ivf(twice, vec), E_ARG + ".*handle with replicas \\(2 devices\\)"),
        (lambda: raw_pq(pq, vec, Q=-1), E_ARG + ".*bad sizes.*Q=-1"),
        (lambda: raw_pq(pq, vec, k=0), E_ARG + ".*bad sizes.*k=0"),
        (lambda: raw_pq(pq, vec, k=5, n_cand=4), E_ARG + ".*bad sizes.*n_cand=4"),
        (lambda: raw_pq(pq, vec, subp=None, ns=3), E_ARG + ".*bad subset.*n_subset=3"),
        (lambda: raw_pq(pq, vec, subp=gpu._p(sub), ns=-1), E_ARG + ".*bad subset.*n_subset=-1"),
        (lambda: raw_pq(pq, vec, tp=None), E_ARG + ".*NULL buffer"),
        (lambda: raw_pq(pq, vec, n_cand=5000), E_LIMIT + ".*n_cand = 5000 exceeds"),
        (lambda: raw_pq(ivf, vec), E_KIND + ".*wrong kind"),
        (lambda: raw_pq(pq, ivf), E_KIND + ".*wrong kind"),
        (lambda: raw_pq(pq, other), E_ARG + ".*vectors have 30 dimensions, the index has 300"),
        (lambda: gpu._check(ivf.lib.freddy_gpu_last_approx_analogy_stats(vec.h, None, None, None)), E_KIND),
    ]
    for call, pattern in refused:
        with pytest.raises(gpu.FreddyGpuError, match=pattern):
            call()
    for idx in (ivf, pq, twice):
        assert idx.profile_read() == {}, "a refused call launched something"
        idx.profile_enable(False)
    other.close()
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
    yield s
    s.close()


def test_host_mirror_batch_equals_the_single_triple_functions(db):
    s = db
    rng = np.random.default_rng(12)
    t = rng.choice(np.arange(1, 20001), (40, 3)).astype(np.int32)
    t[5, 2] = t[5, 0]
    t[0, 1], t[17, 0], t[39, 2] = 20000 + 7, -1, 10**8                            # unknown ids: NULL, -1 here
    inputs = np.concatenate([rng.choice(np.arange(1, 20001), 800, replace=False), np.array([-5, 10**8])]).astype(np.int32)
    for pvf in (1, 6, 20):
        s.set_pvf(pvf)
        for name, batch, single in (
                ("ivfadc", lambda: s.analogy_3cosadd_ivfadc_batch(t), lambda a, b, c: s.analogy_3cosadd_ivfadc(a, b, c)),
                ("pq", lambda: s.analogy_3cosadd_pq_batch(t), lambda a, b, c: s.analogy_3cosadd_pq(a, b, c)),
                ("pq", lambda: s.analogy_3cosadd_in_pq_batch(t, inputs), lambda a, b, c: s.analogy_3cosadd_in_pq(a, b, c, inputs))):
            got = batch()                                                          # (the first call pins google_vecs_norm)
            idx = s.gpu_index(name)
            idx.profile_enable(True)
            got = batch()
            prof = idx.profile_read()
            idx.profile_enable(False)
            assert prof["aa_rerank"][0] == 1 and prof["aa_query"][0] == 1, (name, pvf, prof)   # one device call
            exp = [single(*tr) for tr in t.tolist()]
            assert got.tolist() == exp, (name, pvf)
            assert got[0] == got[17] == got[39] == -1 and (got[1:17] > 0).all()
    s.set_pvf(20)
    assert s.analogy_3cosadd_in_pq_batch(t, []).tolist() == [-1] * 40              # an empty input set: no row, as the single function
    assert s.analogy_3cosadd_in_pq(int(t[1, 0]), int(t[1, 1]), int(t[1, 2]), []) == -1
    assert s.analogy_3cosadd_pq_batch(np.empty((0, 3), np.int32)).size == 0
