"""-m gpu: the batched analogy over the kNN-join (include/freddy_gpu.h: freddy_gpu_ivpq_analogy; the binding IVPQIndex.analogy;
analogy_3cosadd_in_ivpq for a batch of triples).  Expected rows come from the oracle alone (tests/ivpq_analogy_model.py: unit rows ->
ONE Oracle.ivpq_search_in per pass at k = n_cand -> drop the fillers, ids without a vector and the inputs -> exact_knn of RAW over the
rest); a sample of triples is also compared with VectorIndex.search(raw, k, subset_ids=S).  The ivpq handle's profile names aa_query and
aa_rerank once per pass and no query_gather: the unit rows go from aa_query straight into the join's query block."""
import ctypes as C

import numpy as np
import pytest

import approx_analogy_model as am
import ivpq_analogy_model as im
import join_ids_inputs as ji
import pv_model as pm
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND, E_LIMIT = "freddy_gpu error -1", "freddy_gpu error -4", "freddy_gpu error -5"
SETS = ("all", "base300", "base3", "inputs7", "inputs7+2")


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def main(gpu, oracle):
    x, ids, t = ji.analogy_tables()
    h = {"x": x, "ids": ids, "t": am.main_triples(), "ivpq": gpu.IVPQIndex(*ji.pin_args(t)), "vec": gpu.VectorIndex(ids, x),
         "table": oracle.ivpq_table(*ji.pin_args(t)), "sets": ji.analogy_target_sets()}
    yield h
    h["ivpq"].close()
    h["vec"].close()


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    prof = idx.profile_read()
    idx.profile_enable(False)
    return out, prof


def _model(main, oracle, name, method, k, n_cand, triples=None, analogy_pass=0):
    tg, (alpha, pvf, conf) = main["sets"][name]
    return im.expected(oracle, main["table"], main["x"], main["ids"], main["t"] if triples is None else triples, k, n_cand, tg, alpha, pvf, method,
                       confidence=conf, analogy_pass=analogy_pass)


def _call(main, name, method, k, n_cand, triples=None):
    tg, (alpha, pvf, conf) = main["sets"][name]
    return main["ivpq"].analogy(main["vec"], main["t"] if triples is None else triples, k, n_cand, target_ids=tg, alpha=alpha, pvf=pvf, method=method,
                                confidence=conf)


def _same_as_search(vec, vec_ids, triples, k, lists, raw, valid, gi, gs, sample, what):
    """rows of the sample equal VectorIndex.search(raw, k, subset_ids=S)"""
    pos = np.cumsum(valid) - 1
    for q in sample:
        if not valid[q]:
            continue
        _, have = pm.candidates(lists[pos[q]], vec_ids)
        S = have[~np.isin(have, triples[q])]
        si, ss = vec.search(raw[pos[q]], k, subset_ids=S if S.size else np.array([-1], np.int32))
        assert np.array_equal(gi[q], si[0]) and np.array_equal(gs[q].view(np.uint32), ss[0].view(np.uint32)), (what, q)


@pytest.mark.parametrize("k,n_cand", ji.AN_SHAPES)
@pytest.mark.parametrize("method", ji.METHODS)
def test_target_sets(main, oracle, method, k, n_cand):
    ivpq, vec, t = main["ivpq"], main["vec"], main["t"]
    for name in SETS:
        what = f"{name} method={method} k={k} n_cand={n_cand}"
        exp, stats, lists, raw, valid, iters = _model(main, oracle, name, method, k, n_cand)
        (gi, gs), prof = _profiled(ivpq, lambda: _call(main, name, method, k, n_cand))
        pm.same(gi, gs, exp, k, what)
        assert ivpq.last_approx_analogy_stats() == stats, what
        assert set(prof) == {"aa_query", "aa_rerank"} and prof["aa_query"][0] == 1 and prof["aa_rerank"][0] == 1, (what, sorted(prof))
        _same_as_search(vec, main["ids"], t, k, lists, raw, valid, gi, gs, (0, 5, 7, 60, 100, 199), what)
        if name == "inputs7":
            assert (gi[7] == -1).all() and np.isneginf(gs[7]).all(), what          # an empty candidate set


def test_passes_of_64_triples(main, oracle):
    ivpq = main["ivpq"]
    k, n_cand = 3, 23
    ivpq.set_option("analogy_pass", 64)
    try:
        for name, method in (("all", 0), ("base300", 2)):
            exp, stats, lists, raw, valid, iters = _model(main, oracle, name, method, k, n_cand, analogy_pass=64)
            assert len(iters) == 4                                                   # 200 live triples: 64 + 64 + 64 + 8
            (gi, gs), prof = _profiled(ivpq, lambda: _call(main, name, method, k, n_cand))
            pm.same(gi, gs, exp, k, f"analogy_pass=64 {name}")
            assert ivpq.last_approx_analogy_stats() == stats
            assert set(prof) == {"aa_query", "aa_rerank"} and prof["aa_query"][0] == 4 and prof["aa_rerank"][0] == 4, prof
    finally:
        ivpq.set_option("analogy_pass", 0)


def test_unknown_ids(main, oracle):
    """A triple with an unknown id at the first, a middle and the last position: its row is (-1, -inf), its neighbours' rows are what
    they are without it; a batch of unknown triples alone launches nothing."""
    ivpq = main["ivpq"]
    t = main["t"][:70].copy()
    clean_i, clean_s = _call(main, "all", 1, 3, 23, t)
    t[0, 1], t[31, 0], t[69, 2] = 10**8, -7, 20001
    bad = np.array([0, 31, 69])
    exp, stats, _, _, valid, _ = _model(main, oracle, "all", 1, 3, 23, t)
    assert (~valid).nonzero()[0].tolist() == bad.tolist() and stats["searched"] == 67
    (gi, gs), prof = _profiled(ivpq, lambda: _call(main, "all", 1, 3, 23, t))
    pm.same(gi, gs, exp, 3, "unknown ids")
    assert (gi[bad] == -1).all() and np.isneginf(gs[bad]).all()
    ok = np.setdiff1d(np.arange(70), bad)
    assert np.array_equal(gi[ok], clean_i[ok]) and np.array_equal(gs[ok].view(np.uint32), clean_s[ok].view(np.uint32))
    assert ivpq.last_approx_analogy_stats() == stats and prof["aa_rerank"][0] == 1
    (gi, gs), prof = _profiled(ivpq, lambda: _call(main, "all", 1, 3, 23, t[bad]))
    assert (gi == -1).all() and np.isneginf(gs).all() and gi.shape == (3, 3) and prof == {}
    assert ivpq.last_approx_analogy_stats() == {"searched": 0, "candidates": 0, "scored": 0}
    gi, gs = _call(main, "all", 1, 3, 23, np.empty((0, 3), np.int32))               # Q = 0
    assert gi.shape == (0, 3) and ivpq.last_approx_analogy_stats() == {"searched": 0, "candidates": 0, "scored": 0}


def test_interleaved_with_the_joins(main, oracle):
    """analogy, knn_join and knn_join_ids share the handle's query block and target-list cache: interleaved, each returns what it returns alone"""
    ivpq, vec, x, ids = main["ivpq"], main["vec"], main["x"], main["ids"]
    tg, (alpha, pvf, conf) = main["sets"]["base300"]
    rows = np.sort(np.random.default_rng(8).choice(ids.size, 300, replace=False))
    jexp, jit = oracle.ivpq_search_in(main["table"], x[rows], 5, tg, alpha, pvf, 0, confidence=conf)
    aexp, astats, *_ = _model(main, oracle, "base300", 0, 1, 4)
    for _ in range(2):
        gi, gs = _call(main, "base300", 0, 1, 4)
        pm.same(gi, gs, aexp, 1, "interleaved: analogy")
        fi, fd, fit = ivpq.knn_join(x[rows], 5, tg, alpha, pvf, 0, confidence=conf)
        util.assert_same_lists(fi, fd, jexp, "interleaved: knn_join")
        gi, gs = _call(main, "base300", 0, 1, 4)
        pm.same(gi, gs, aexp, 1, "interleaved: analogy after knn_join")
        gq, ji_, jd, git = ivpq.knn_join_ids(vec, ids[rows], 5, tg, alpha, pvf, 0, confidence=conf)
        util.assert_same_lists(ji_, jd, jexp, "interleaved: knn_join_ids")
        assert fit == git == jit


def test_refusals(gpu, main):
    ivpq, vec = main["ivpq"], main["vec"]
    lib, P = ivpq.lib, gpu._p
    t = main["t"][:3].copy()
    tg = main["sets"]["base300"][0]
    oi, os_ = np.full((3, 2), -77, np.int32), np.full((3, 2), -77.0, np.float32)
    other = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), util.shape_corpus(6000, 30).numpy()[:100])

    def call(a=ivpq.h, v=vec.h, tr=P(t), Q=3, k=2, n_cand=4, tids=P(tg), nt=tg.size, alpha=1, pvf=3, method=0, oi_=P(oi), os2=P(os_)):
        return lib.freddy_gpu_ivpq_analogy(a, v, tr, Q, k, n_cand, tids, nt, alpha, pvf, method, 1, C.c_float(0.8), 10000000, oi_, os2)

    table = [
        (dict(Q=-1), E_ARG, "bad sizes"), (dict(k=0), E_ARG, "bad sizes"), (dict(k=5), E_ARG, "bad sizes"), (dict(tr=None), E_ARG, "NULL buffer"),
        (dict(oi_=None), E_ARG, "NULL buffer"), (dict(n_cand=4097), E_LIMIT, "n_cand = 4097"),
        (dict(a=None), E_ARG, "NULL index"), (dict(v=None), E_ARG, "NULL index"),
        (dict(nt=-1), E_ARG, "bad sizes"), (dict(tids=None), E_ARG, "NULL target ids"), (dict(method=3), E_ARG, "Unknown computation method!"),
        (dict(n_cand=2049, method=2, pvf=4), E_LIMIT, "k\\*pvf=8196"),
        (dict(a=vec.h), E_KIND, "wrong kind"), (dict(v=ivpq.h), E_KIND, "wrong kind"),
        (dict(v=other.h), E_ARG, "vectors have 30 dimensions, the index has 300"),
        # the order: the analogy's scalars, then the join's checks, then the handles
        (dict(k=0, method=3, a=vec.h), E_ARG, "bad sizes \\(Q=3"), (dict(method=3, a=vec.h), E_ARG, "Unknown computation"),
    ]
    try:
        ivpq.profile_enable(True)
        c0 = gpu.alloc_stats().calls
        for kw, code, msg in table:
            with pytest.raises(gpu.FreddyGpuError, match=code + ".*" + msg):
                gpu._check(call(**kw))
        assert gpu.alloc_stats().calls == c0, "a refused call allocated"
        assert ivpq.profile_read() == {}, "a refused call launched something"
        ivpq.profile_enable(False)
        assert (oi == -77).all() and (os_ == -77.0).all()
        with pytest.raises(gpu.FreddyGpuError, match=E_KIND):
            vec.last_approx_analogy_stats()                                          # the vector handle stays refused
    finally:
        other.close()
