"""-m gpu: searches by row id (include/freddy_gpu.h: freddy_gpu_ivfadc_search_ids, freddy_gpu_pq_search_ids and their _pv forms; the
bindings search_ids / search_pv_ids).  The queries are rows of a pinned vector table, selected by the id rule on the host and gathered
on the device (csrc/query_ids.h query_gather_kernel).

Expected lists come from the oracle alone, over the vectors x[row] that a numpy model of the id rule selects (tests/query_ids_inputs.py:
model); a sample of queries is also compared with the existing entry point called with those host vectors.  The ANN handle's profile
names the kernels that ran: ONE query runs exactly the kernels of the plain search (it is read where its row lies), more than one run
them and query_gather; a call that selects nothing leaves an empty profile.
Tables: 6000 .. 20 000 rows, a vector table of 4999 rows with the ids 3 r + 1."""
import ctypes as C

import numpy as np
import pytest

import dev_contract_inputs as dci
import pv_model as pm
import query_ids_inputs as qi
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND, E_LIMIT = "freddy_gpu error -1", "freddy_gpu error -4", "freddy_gpu error -5"
TO, POS = qi.TABLE_ORDER, qi.POSITIONAL


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


def _same(gi, gd, exp, what):
    util.assert_same_lists(gi, gd, exp, what)


def _fillers(gi, gd, slots, value, what):
    assert (gi[slots] == -1).all(), what
    v = gd[slots]
    assert (np.isneginf(v).all() if np.isneginf(value) else (v == np.float32(value)).all()), what


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    """every shape's handles, pinned once: ivf, vec (and pq for the 300-d / K = 256 shape), the oracle's tables"""
    out = {}
    for shape in qi.SHAPES:
        c = qi.case(shape)
        h = {"c": c, "ivf": gpu.IVFIndex(*qi.ivf_args(c["ivf"])), "vec": gpu.VectorIndex(c["vec_ids"], c["vec_x"]),
             "ivf_t": oracle.ivf_table(*qi.ivf_args(c["ivf"]))}
        if "pq" in c:
            h["pq"] = gpu.PQIndex(c["pq"]["codebook"], c["pq"]["ids"], c["pq"]["codes"])
            h["pq_t"] = oracle.pq_table(c["pq"]["codebook"], c["pq"]["ids"], c["pq"]["codes"])
        out[shape] = h
    yield out
    for h in out.values():
        for n in ("ivf", "vec", "pq"):
            if n in h:
                h[n].close()


# ---- shapes x query counts x both rules ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", qi.SHAPES)
def test_counts_and_rules(cases, oracle, shape):
    h = cases[shape]
    c, ivf, vec = h["c"], h["ivf"], h["vec"]
    vids, vx, W, k = c["vec_ids"], c["vec_x"], c["W"], 5
    for n in qi.COUNTS:
        known = qi.known_ids(vids, n, seed=n)
        noisy = qi.noisy_ids(vids, known, seed=n)
        # TABLE_ORDER over the noisy array: n queries, ascending
        sel, rows = qi.model(vids, noisy, TO)
        assert sel.size == n
        exp = oracle.ivfadc_search_many(h["ivf_t"], vx[rows], k, W, sentinel=1000.0, found_rule=0)
        what = f"{shape} n={n} table order"
        (hi, hd), plain = _profiled(ivf, lambda: ivf.search(vx[rows], k, W))
        (gq, gi, gd), names = _profiled(ivf, lambda: ivf.search_ids(vec, noisy, k, W, rule=TO))
        assert np.array_equal(gq, sel), what
        _same(gi, gd, exp, what)
        assert np.array_equal(gi, hi) and np.array_equal(gd.view(np.uint32), hd.view(np.uint32)), what   # the existing entry point, host vectors
        assert names == (plain if n == 1 else plain | {"query_gather"}), (what, sorted(names), sorted(plain))
        # POSITIONAL over the same array: every slot, fillers where there is no row, a repeated id answered again
        sel, rows = qi.model(vids, noisy, POS)
        live = rows >= 0
        exp = oracle.ivfadc_search_many(h["ivf_t"], vx[rows[live]], k, W, sentinel=100.0, found_rule=1)
        what = f"{shape} n={n} positional"
        gq, gi, gd = ivf.search_ids(vec, noisy, k, W, sentinel=100.0, found_rule=1, rule=POS)
        assert np.array_equal(gq, noisy) and gi.shape == (noisy.size, k), what
        _same(gi[live], gd[live], exp, what)
        _fillers(gi, gd, ~live, 100.0, what)
        # POSITIONAL over the known ids alone: exactly n queries (no compaction), in the caller's order
        sel, rows = qi.model(vids, known, POS)
        exp = oracle.ivfadc_search_many(h["ivf_t"], vx[rows], k, W, sentinel=1000.0, found_rule=0)
        (gq, gi, gd), names = _profiled(ivf, lambda: ivf.search_ids(vec, known, k, W, rule=POS))
        assert np.array_equal(gq, known), what
        _same(gi, gd, exp, f"{shape} n={n} positional, known ids")
        assert ("query_gather" in names) == (n > 1), (what, sorted(names))
    assert ivf.bound_violations() == 0


def test_only_unknown_ids_launch_nothing(cases):
    h = cases["d300_k256"]
    ivf, pq, vec, vids = h["ivf"], h["pq"], h["vec"], h["c"]["vec_ids"]
    unknown = np.array([0, -3, vids[5] + 1, vids[-1] + 1, 2 ** 30], np.int32)
    for idx, call, filler in ((ivf, lambda r: ivf.search_ids(vec, unknown, 5, 4, rule=r), 1000.0),
                              (pq, lambda r: pq.search_ids(vec, unknown, 5, rule=r), 100.0),
                              (ivf, lambda r: ivf.search_pv_ids(vec, unknown, 5, 6, 4, rule=r), -np.inf),
                              (pq, lambda r: pq.search_pv_ids(vec, unknown, 5, 6, rule=r), -np.inf)):
        (gq, gi, gd), names = _profiled(idx, lambda: call(TO))
        assert gq.size == 0 and gi.shape == (0, 5) and names == set()
        (gq, gi, gd), names = _profiled(idx, lambda: call(POS))
        assert np.array_equal(gq, unknown) and names == set()
        _fillers(gi, gd, np.ones(unknown.size, bool), filler, "only unknown ids")
    (gq, gi, gd), names = _profiled(ivf, lambda: ivf.search_ids(vec, np.empty(0, np.int32), 5, 4))
    assert gq.size == 0 and gi.shape == (0, 5) and names == set()              # n_ids == 0 succeeds


def test_table_order_leaves_the_slots_beyond_q_alone(gpu, cases, oracle):
    """The C call itself (the binding cuts its arrays to n_queries): the buffers hold n_ids slots, TABLE_ORDER fills the first Q."""
    h = cases["d300_k256"]
    c, ivf, vec = h["c"], h["ivf"], h["vec"]
    noisy = qi.noisy_ids(c["vec_ids"], qi.known_ids(c["vec_ids"], 9, seed=3), seed=3)
    sel, rows = qi.model(c["vec_ids"], noisy, TO)
    n, k = noisy.size, 5
    oq, oi, od = np.full(n, -77, np.int32), np.full((n, k), -77, np.int32), np.full((n, k), -77.0, np.float32)
    nq = C.c_int32(-1)
    P = gpu._p
    gpu._check(ivf.lib.freddy_gpu_ivfadc_search_ids(ivf.h, vec.h, P(noisy), n, TO, k, 4, C.c_float(1000.0), 0, P(oq), C.byref(nq), P(oi), P(od)))
    Q = nq.value
    assert Q == sel.size < n and np.array_equal(oq[:Q], sel)
    _same(oi[:Q], od[:Q], oracle.ivfadc_search_many(h["ivf_t"], c["vec_x"][rows], k, 4, sentinel=1000.0, found_rule=0), "the first Q slots")
    assert (oq[Q:] == -77).all() and (oi[Q:] == -77).all() and (od[Q:] == -77.0).all()


# ---- pipelined sub-batches, stragglers, k > 512 ----------------------------------------------------------------------------------
def test_pipelined_sub_batches(cases, oracle):
    """pipeline_batch = 64, four lanes, Q = 64 * 9 + 5: ten sub-batches, every lane slot is used again and the last one is short"""
    h = cases["d300_k256"]
    c, ivf, vec = h["c"], h["ivf"], h["vec"]
    Q = 64 * 9 + 5
    known = qi.known_ids(c["vec_ids"], Q, seed=77)
    sel, rows = qi.model(c["vec_ids"], known, POS)
    exp = oracle.ivfadc_search_many(h["ivf_t"], c["vec_x"][rows], 5, 4, sentinel=1000.0, found_rule=0, n_threads=8)
    ivf.set_option("pipeline_batch", 64); ivf.set_option("pipeline_lanes", 4)
    try:
        (gq, gi, gd), names = _profiled(ivf, lambda: ivf.search_ids(vec, known, 5, 4, rule=POS))
    finally:
        ivf.set_option("pipeline_batch", 2048)
    assert np.array_equal(gq, known)
    _same(gi, gd, exp, "pipelined sub-batches")
    assert "query_gather" in names


@pytest.mark.parametrize("W,rule,sentinel", qi.straggler_runs())
def test_stragglers(gpu, W, rule, sentinel):
    """Round one leaves queries unfinished (tests/test_query_ids_inputs_cpu.py): the re-search gathers them again from the device.  One
    sub-batch, and sub-batches of 64."""
    s = qi.straggler_case(W)
    c, k = s["c"], qi.STRAGGLER_KEY[2]
    exp = dci.search(c, s["vec_x"], k, W, rule, 0, sentinel=sentinel)[0]
    ivf = gpu.IVFIndex(*qi.ivf_args(c))
    vec = gpu.VectorIndex(s["vec_ids"], s["vec_x"])
    ids = s["vec_ids"][np.random.default_rng(4).permutation(s["vec_ids"].size)]
    try:
        for batch in (2048, 64):
            ivf.set_option("pipeline_batch", batch)
            gq, gi, gd = ivf.search_ids(vec, ids, k, W, sentinel=sentinel, found_rule=rule, rule=TO)
            assert np.array_equal(gq, s["vec_ids"])
            _same(gi, gd, exp, f"stragglers W={W} rule={rule} pipeline_batch={batch}")
            gq, gi, gd = ivf.search_ids(vec, ids, k, W, sentinel=sentinel, found_rule=rule, rule=POS)
            order = (ids - 1) // 3
            _same(gi, gd, exp[order], f"stragglers positional W={W} rule={rule} pipeline_batch={batch}")
    finally:
        ivf.close()
        vec.close()


def test_k_600(cases, oracle):
    h = cases["d300_k256"]
    c, ivf, vec = h["c"], h["ivf"], h["vec"]
    known = qi.known_ids(c["vec_ids"], 9, seed=600)
    sel, rows = qi.model(c["vec_ids"], known, TO)
    exp = oracle.ivfadc_search_many(h["ivf_t"], c["vec_x"][rows], 600, 4, sentinel=1000.0, found_rule=0, n_threads=8)
    (gq, gi, gd), names = _profiled(ivf, lambda: ivf.search_ids(vec, known, 600, 4))
    assert np.array_equal(gq, sel)
    _same(gi, gd, exp, "k = 600")
    assert {"merge_select", "bigk_replay", "query_gather"} <= names, sorted(names)


# ---- PQ --------------------------------------------------------------------------------------------------------------------------
def test_pq(cases, oracle):
    h = cases["d300_k256"]
    c, pq, vec = h["c"], h["pq"], h["vec"]
    vids, vx = c["vec_ids"], c["vec_x"]
    rng = np.random.default_rng(3)
    subset = rng.permutation(np.concatenate([c["pq"]["ids"][rng.choice(20000, 6000, replace=False)], np.array([-5, 0, 10 ** 8], np.int32)])).astype(np.int32)
    for n in (1, 9, 70):
        noisy = qi.noisy_ids(vids, qi.known_ids(vids, n, seed=50 + n), seed=n)
        for sub, sentinel in ((None, 100.0), (subset, 1000.0)):
            what = f"pq n={n} subset={sub is not None}"
            sel, rows = qi.model(vids, noisy, TO)
            qs = vx[rows]
            exp = np.stack([oracle.pq_search(h["pq_t"], q, 5) if sub is None else oracle.pq_search_in(h["pq_t"], q, 5, sub) for q in qs])
            (hi, hd), plain = _profiled(pq, lambda: pq.search(qs, 5, sentinel=sentinel, subset_ids=sub))
            (gq, gi, gd), names = _profiled(pq, lambda: pq.search_ids(vec, noisy, 5, sentinel=sentinel, subset_ids=sub))
            assert np.array_equal(gq, sel), what
            _same(gi, gd, exp, what)
            assert np.array_equal(gi, hi) and np.array_equal(gd.view(np.uint32), hd.view(np.uint32)), what
            assert names == (plain if n == 1 else plain | {"query_gather"}), (what, sorted(names), sorted(plain))
            sel, rows = qi.model(vids, noisy, POS)
            live = rows >= 0
            gq, gi, gd = pq.search_ids(vec, noisy, 5, sentinel=sentinel, subset_ids=sub, rule=POS)
            assert np.array_equal(gq, noisy), what
            order = np.searchsorted(np.sort(np.unique(noisy[live])), noisy[live])
            _same(gi[live], gd[live], exp[order], what + " positional")
            _fillers(gi, gd, ~live, sentinel, what + " positional")


# ---- post verification -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pv(gpu, oracle):
    x, ids, qs, ivf, pq = pm.main_tables()
    h = {"x": x, "ids": ids, "ivf": gpu.IVFIndex(*qi.ivf_args(ivf)), "pq": gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"]),
         "vec": gpu.VectorIndex(ids, x), "ivf_t": oracle.ivf_table(*qi.ivf_args(ivf)), "pq_t": oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])}
    yield h
    for n in ("ivf", "pq", "vec"):
        h[n].close()


def _pv_ids(ids, n, seed):
    """query ids over pv_model's table (ids 1 .. N): duplicate rows 100 .. 139 among them, noise around them"""
    known = qi.known_ids(ids, n, seed)
    if n >= 9:
        known[2:6] = ids[[100, 101, 10000, 10001]]
        known = known[np.sort(np.unique(known, return_index=True)[1])]
    return known, np.concatenate([[0], known, known[:max(1, n // 4)], [ids[-1] + 5, -1]]).astype(np.int32)


@pytest.mark.parametrize("k,pvf", [(5, 1), (5, 20), (30, 20)])
def test_post_verification(pv, oracle, k, pvf):
    x, ids, ivf, pq, vec = pv["x"], pv["ids"], pv["ivf"], pv["pq"], pv["vec"]
    kc, W = k * pvf, 3
    for n in (1, 70 if k == 5 else 9):
        known, noisy = _pv_ids(ids, n, seed=k + pvf + n)
        sel, rows = qi.model(ids, noisy, TO)
        qs = x[rows]
        what = f"pv ivf k={k} pvf={pvf} n={n}"
        exp, n_cand, n_scored = pm.expected(oracle, pm.ivf_lists(oracle, pv["ivf_t"], qs, kc, W), x, ids, qs, k)
        _, plain = _profiled(ivf, lambda: ivf.search(qs, kc, W))
        (gq, gi, gs), names = _profiled(ivf, lambda: ivf.search_pv_ids(vec, noisy, k, pvf, W))
        assert np.array_equal(gq, sel), what
        pm.same(gi, gs, exp, k, what)
        assert names == plain | {"query_gather", "pv_rerank"}, (what, sorted(names), sorted(plain))
        assert ivf.last_pv_stats() == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())}, what
        hi, hs = ivf.search_pv(vec, qs, k, pvf, W)                               # the existing entry point, host vectors
        assert np.array_equal(gi, hi) and np.array_equal(gs.view(np.uint32), hs.view(np.uint32)), what
        # positional: fillers are (-1, -inf); the counts cover the searched slots
        sel, rows = qi.model(ids, noisy, POS)
        live = rows >= 0
        gq, gi, gs = ivf.search_pv_ids(vec, noisy, k, pvf, W, rule=POS)
        assert np.array_equal(gq, noisy), what
        order = np.searchsorted(np.sort(np.unique(noisy[live])), noisy[live])
        pm.same(gi[live], gs[live], [exp[o] for o in order], k, what + " positional")
        _fillers(gi, gs, ~live, -np.inf, what + " positional")
        assert ivf.last_pv_stats() == {"candidates": int(n_cand[order].sum()), "scored": int(n_scored[order].sum())}, what
        # pq
        what = f"pv pq k={k} pvf={pvf} n={n}"
        sel, rows = qi.model(ids, noisy, TO)
        exp, n_cand, n_scored = pm.expected(oracle, pm.pq_lists(oracle, pv["pq_t"], qs, kc), x, ids, qs, k)
        _, plain = _profiled(pq, lambda: pq.search(qs, kc))
        (gq, gi, gs), names = _profiled(pq, lambda: pq.search_pv_ids(vec, noisy, k, pvf))
        assert np.array_equal(gq, sel), what
        pm.same(gi, gs, exp, k, what)
        assert names == plain | {"query_gather", "pv_rerank"}, (what, sorted(names), sorted(plain))
        assert pq.last_pv_stats() == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())}, what


# ---- after a mutation of the vector table ----------------------------------------------------------------------------------------
def test_after_a_mutation_of_vecs(gpu, cases, oracle):
    h = cases["d300_k256"]
    c, ivf = h["c"], h["ivf"]
    vids, vx = c["vec_ids"].copy(), c["vec_x"].copy()
    vec = gpu.VectorIndex(vids, vx)
    x = pm.main_tables()[0]
    upd, rem, app = int(vids[40]), int(vids[41]), int(vids[-1]) + 3
    query = np.array([vids[39], upd, rem, app, vids[0], 2], np.int32)
    try:
        gq, _, _ = ivf.search_ids(vec, query, 5, 4)
        assert gq.tolist() == sorted([int(vids[39]), upd, rem, int(vids[0])])     # before: the appended id has no row yet
        assert vec.update_rows(np.array([upd], np.int32), vectors=x[12345:12346]) == 1
        assert vec.remove_rows(np.array([rem], np.int32)) == 1
        vec.append_rows(np.array([app], np.int32), vectors=x[15555:15556])
        vx[40] = x[12345]
        keep = np.arange(vids.size) != 41
        vids2, vx2 = np.concatenate([vids[keep], [app]]).astype(np.int32), np.concatenate([vx[keep], x[15555:15556]])
        for rule in (TO, POS):
            sel, rows = qi.model(vids2, query, rule)
            live = rows >= 0
            exp = oracle.ivfadc_search_many(h["ivf_t"], vx2[rows[live]], 5, 4, sentinel=1000.0, found_rule=0)
            gq, gi, gd = ivf.search_ids(vec, query, 5, 4, rule=rule)
            assert np.array_equal(gq, sel) and (rem not in sel.tolist() if rule == TO else not live[2]), rule
            _same(gi[live], gd[live], exp, f"after the mutation, rule {rule}")
            _fillers(gi, gd, ~live, 1000.0, f"after the mutation, rule {rule}")
            assert app in gq.tolist() and upd in gq.tolist()
        # the updated row answers with its new vector, not with the one it was pinned with
        gq, gi, gd = ivf.search_ids(vec, np.array([upd], np.int32), 5, 4)
        old = oracle.ivfadc_search_many(h["ivf_t"], c["vec_x"][40:41], 5, 4)
        assert not np.array_equal(gi, old["id"])
    finally:
        vec.close()


# ---- refusals: every line of the header's table, its message, nothing launched -----------------------------------------------------
def test_refusals(gpu, cases):
    h = cases["d300_k256"]
    ivf, pq, vec = h["ivf"], h["pq"], h["vec"]
    lib, f = ivf.lib, C.c_float
    q = np.array([1, 4, 7], np.int32)
    oq, oi, od = np.empty(3, np.int32), np.empty((3, 5), np.int32), np.empty((3, 5), np.float32)
    nq = C.c_int32(-9)
    P = gpu._p

    def ivf_ids(a=ivf.h, v=vec.h, ids=P(q), n=3, rule=0, k=5, W=4, fr=0, oq_=P(oq), nq_=C.byref(nq), oi_=P(oi), od_=P(od)):
        return lib.freddy_gpu_ivfadc_search_ids(a, v, ids, n, rule, k, W, f(1000.0), fr, oq_, nq_, oi_, od_)

    def pq_ids(a=pq.h, v=vec.h, ids=P(q), n=3, rule=0, k=5, sub=None, ns=0, oq_=P(oq), nq_=C.byref(nq), oi_=P(oi), od_=P(od)):
        return lib.freddy_gpu_pq_search_ids(a, v, ids, n, rule, k, f(100.0), sub, ns, oq_, nq_, oi_, od_)

    def ivf_pv(a=ivf.h, v=vec.h, ids=P(q), n=3, rule=0, k=5, pvf=6, W=4, fr=0, oq_=P(oq), nq_=C.byref(nq), oi_=P(oi), od_=P(od)):
        return lib.freddy_gpu_ivfadc_search_pv_ids(a, v, ids, n, rule, k, pvf, W, f(1000.0), fr, oq_, nq_, oi_, od_)

    def pq_pv(a=pq.h, v=vec.h, ids=P(q), n=3, rule=0, k=5, pvf=6, sub=None, ns=0, oq_=P(oq), nq_=C.byref(nq), oi_=P(oi), od_=P(od)):
        return lib.freddy_gpu_pq_search_pv_ids(a, v, ids, n, rule, k, pvf, f(100.0), sub, ns, oq_, nq_, oi_, od_)

    other = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), util.shape_corpus(6000, 30).numpy()[:100])
    twice = gpu.IVFIndex(*qi.ivf_args(h["c"]["ivf"]), devices=[0, 0])
    every = (ivf_ids, pq_ids, ivf_pv, pq_pv)
    table = [(fn, kw, code, msg) for fn in every for kw, code, msg in (
        (dict(a=None), E_ARG, "NULL index"), (dict(v=None), E_ARG, "NULL index"), (dict(n=-1), E_ARG, "n_ids=-1"),
        (dict(rule=2), E_ARG, "bad id_rule 2"), (dict(rule=-1), E_ARG, "bad id_rule -1"), (dict(nq_=None), E_ARG, "NULL n_queries"),
        (dict(ids=None), E_ARG, "NULL buffer"), (dict(oq_=None), E_ARG, "NULL buffer"), (dict(oi_=None), E_ARG, "NULL buffer"),
        (dict(od_=None), E_ARG, "NULL buffer"), (dict(v=other.h), E_ARG, "vectors have 30 dimensions, the index has 300"),
        (dict(v=ivf.h), E_KIND, "wrong kind"), (dict(a=vec.h), E_KIND, "wrong kind"))]
    table += [(fn, dict(k=0), E_ARG, "k > 0") for fn in (ivf_ids, pq_ids)] + [(fn, dict(k=4097), E_LIMIT, "k=4097") for fn in (ivf_ids, pq_ids)]
    table += [(fn, dict(k=0), E_ARG, "bad sizes") for fn in (ivf_pv, pq_pv)] + [(fn, dict(pvf=0), E_ARG, "bad sizes") for fn in (ivf_pv, pq_pv)]
    table += [(fn, dict(k=100, pvf=41), E_LIMIT, "k \\* pvf = 4100") for fn in (ivf_pv, pq_pv)]
    table += [(fn, dict(W=0), E_ARG, "W must be positive") for fn in (ivf_ids, ivf_pv)]
    table += [(fn, dict(fr=3), E_ARG, "bad found_rule") for fn in (ivf_ids, ivf_pv)] + [(fn, dict(fr=2, W=4), E_ARG, "bad found_rule") for fn in (ivf_ids, ivf_pv)]
    table += [(fn, dict(ns=-1), E_ARG, "bad subset") for fn in (pq_ids, pq_pv)] + [(fn, dict(ns=3), E_ARG, "bad subset") for fn in (pq_ids, pq_pv)]
    table += [(fn, dict(a=pq.h), E_KIND, "wrong kind") for fn in (ivf_ids, ivf_pv)] + [(fn, dict(a=ivf.h), E_KIND, "wrong kind") for fn in (pq_ids, pq_pv)]
    table += [(fn, dict(a=twice.h), E_ARG, "handle with replicas \\(2 devices\\)") for fn in (ivf_ids, ivf_pv)]
    # the order of the table: the front checks before the scalars, the scalars before the kinds, the kinds before the shapes
    table += [(ivf_ids, dict(rule=5, k=0, a=pq.h), E_ARG, "bad id_rule 5"), (ivf_ids, dict(k=0, a=pq.h), E_ARG, "k > 0"),
              (ivf_ids, dict(W=0, a=pq.h), E_ARG, "W must be positive"), (pq_pv, dict(pvf=0, a=ivf.h, v=other.h), E_ARG, "bad sizes"),
              (pq_ids, dict(a=ivf.h, v=other.h), E_KIND, "wrong kind")]
    try:
        for idx in (ivf, pq, twice):
            idx.profile_enable(True)
        for fn, kw, code, msg in table:
            nq.value = -9
            with pytest.raises(gpu.FreddyGpuError, match=code + ".*" + msg):
                gpu._check(fn(**kw))
            assert nq.value == -9, (fn.__name__, kw)                             # nothing written
        for idx in (ivf, pq, twice):
            assert set(idx.profile_read()) == set(), "a refused call launched something"
            idx.profile_enable(False)
        assert ivf_ids(n=0, ids=None, oq_=None, oi_=None, od_=None) == 0 and nq.value == 0      # n_ids == 0 succeeds
        nq.value = -9
        assert pq_pv(n=0) == 0 and nq.value == 0
    finally:
        other.close()
        twice.close()


# ---- poisoned handles: refused as everywhere, before anything is launched or allocated ---------------------------------------------
UNPIN = "unpin it and pin again"


def _poisoned(gpu, make, mutate, probe):
    """A handle that a failed mutation has poisoned: update_rows writes in place, so one of its allocations -- counted first on a
    handle of its own -- fails after the first write.  Tried from the last allocation down.  probe: the kind's plain search with
    k = 0, refused before anything is launched in either state -- FREDDY_E_HIP with the unpin message by a poisoned handle,
    FREDDY_E_ARG by a healthy one (tests/test_gpu_alloc_failures.py)."""
    ref = make()
    c0 = gpu.alloc_stats().calls
    mutate(ref)
    A = gpu.alloc_stats().calls - c0
    ref.close()
    lib = gpu.load()
    for n in range(A, 0, -1):
        h = make()
        gpu.alloc_fail_nth(n)
        try:
            mutate(h)
        except gpu.FreddyGpuError as e:
            assert e.code == gpu.E_NOMEM, e
        finally:
            gpu.alloc_fail_nth(0)
        rc = probe(h)
        assert rc in (-1, -2), rc
        if rc == -2:
            assert UNPIN in lib.freddy_gpu_last_error().decode()
            return h
        h.close()
    raise AssertionError(f"none of the {A} allocations of update_rows, failed, poisons the handle")


@pytest.mark.parametrize("which", ["ivf", "pq", "vecs"])
def test_poisoned_handles_are_refused(gpu, cases, which):
    """A poisoned ivf, pq or vector handle through every *_ids entry point that takes it: FREDDY_E_HIP with the unpin message, after
    the scalar checks (k = 0 is still FREDDY_E_ARG) and before the ids are looked up; an empty profile on both handles, no allocation,
    n_queries and the buffers untouched."""
    c = qi.case("d300_k256")
    ivf_t, pq_t, vids, vx = c["ivf"], c["pq"], c["vec_ids"], c["vec_x"]
    cell = np.repeat(np.arange(ivf_t["list_off"].size - 1), np.diff(ivf_t["list_off"])).astype(np.int32)
    lib, f, P = gpu.load(), C.c_float, gpu._p
    one_q, o1, o2 = vx[:1], np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
    if which == "ivf":
        bad = _poisoned(gpu, lambda: gpu.IVFIndex(*qi.ivf_args(ivf_t)),
                        lambda h: h.update_rows(ivf_t["ids"][:40], coarse_id=cell[40:80], codes=ivf_t["codes"][40:80]),
                        lambda h: lib.freddy_gpu_ivfadc_search(h.h, P(one_q), 1, 0, 3, f(1000.0), 0, P(o1), P(o2)))
        ivf, pq, vec = bad, None, cases["d300_k256"]["vec"]
    elif which == "pq":
        bad = _poisoned(gpu, lambda: gpu.PQIndex(pq_t["codebook"], pq_t["ids"], pq_t["codes"]), lambda h: h.update_rows(pq_t["ids"][:40], codes=pq_t["codes"][40:80]),
                        lambda h: lib.freddy_gpu_pq_search(h.h, P(one_q), 1, 0, f(100.0), None, 0, P(o1), P(o2)))
        ivf, pq, vec = None, bad, cases["d300_k256"]["vec"]
    else:
        bad = _poisoned(gpu, lambda: gpu.VectorIndex(vids, vx), lambda h: h.update_rows(vids[:40], vectors=vx[40:80]),
                        lambda h: lib.freddy_gpu_exact_search(h.h, P(one_q), 1, 0, None, 0, P(o1), P(o2)))
        ivf, pq, vec = cases["d300_k256"]["ivf"], cases["d300_k256"]["pq"], bad
    q = qi.known_ids(vids, 9, seed=1)
    oq, oi, od = np.full(9, -77, np.int32), np.full((9, 5), -77, np.int32), np.full((9, 5), -77.0, np.float32)
    nq = C.c_int32(-9)
    calls = []
    if ivf is not None:
        calls += [lambda k: lib.freddy_gpu_ivfadc_search_ids(ivf.h, vec.h, P(q), 9, TO, k, 4, f(1000.0), 0, P(oq), C.byref(nq), P(oi), P(od)),
                  lambda k: lib.freddy_gpu_ivfadc_search_pv_ids(ivf.h, vec.h, P(q), 9, POS, k, 1, 4, f(1000.0), 0, P(oq), C.byref(nq), P(oi), P(od))]
    if pq is not None:
        calls += [lambda k: lib.freddy_gpu_pq_search_ids(pq.h, vec.h, P(q), 9, POS, k, f(100.0), None, 0, P(oq), C.byref(nq), P(oi), P(od)),
                  lambda k: lib.freddy_gpu_pq_search_pv_ids(pq.h, vec.h, P(q), 9, TO, k, 1, f(100.0), None, 0, P(oq), C.byref(nq), P(oi), P(od))]
    anns = [h for h in (ivf, pq) if h is not None]
    try:
        for h in anns:
            h.profile_enable(True)
        c0 = gpu.alloc_stats().calls
        for call in calls:
            assert call(5) == -2, lib.freddy_gpu_last_error()                       # FREDDY_E_HIP
            assert UNPIN in lib.freddy_gpu_last_error().decode()
            assert call(0) == -1                                                    # the scalars are checked first
        assert gpu.alloc_stats().calls == c0, "a refused call allocated"
        for h in anns:
            assert set(h.profile_read()) == set(), "a refused call launched something"
            h.profile_enable(False)
        assert nq.value == -9 and (oq == -77).all() and (oi == -77).all() and (od == -77.0).all()
    finally:
        bad.close()


# ---- allocation failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ivf", "pq", "ivf_pv"])
def test_allocation_failures(gpu, oracle, form):
    """On fresh handles the n-th allocation of the first call fails, for every n the call makes: FREDDY_E_NOMEM, and the same call made
    again returns the oracle's lists."""
    c = qi.case("d300_k256")
    vids, vx = c["vec_ids"], c["vec_x"]
    query = qi.noisy_ids(vids, qi.known_ids(vids, 20, seed=9), seed=9)
    sel, rows = qi.model(vids, query, TO)
    if form == "pq":
        N = 4200
        args = (c["pq"]["codebook"], c["pq"]["ids"][:N], c["pq"]["codes"][:N])
        t = oracle.pq_table(*args)
        exp = np.stack([oracle.pq_search(t, q, 5) for q in vx[rows]])
        make = lambda: gpu.PQIndex(*args)
        call = lambda a, v: a.search_ids(v, query, 5)
    else:
        exp = oracle.ivfadc_search_many(oracle.ivf_table(*qi.ivf_args(c["ivf"])), vx[rows], 5 if form == "ivf" else 30, 4, sentinel=1000.0, found_rule=0)
        make = lambda: gpu.IVFIndex(*qi.ivf_args(c["ivf"]))
        if form == "ivf":
            call = lambda a, v: a.search_ids(v, query, 5, 4)
        else:
            lists = exp["id"]     # stage one at k * pvf = 30; re-ranked against the vector table itself, which holds every third id
            call = lambda a, v: a.search_pv_ids(v, query, 5, 6, 4)

    def check(res):
        assert np.array_equal(res[0], sel)
        if form == "ivf_pv":
            e, _, _ = pm.expected(oracle, lists, vx, vids, vx[rows], 5)
            pm.same(res[1], res[2], e, 5, form)
        else:
            _same(res[1], res[2], exp, form)

    gpu.alloc_fail_nth(0)
    a, v = make(), gpu.VectorIndex(vids, vx)
    c0 = gpu.alloc_stats().calls
    check(call(a, v))
    A = gpu.alloc_stats().calls - c0
    a.close(); v.close()
    assert A >= 4, f"{form}: {A} allocations through the seam"
    for n in range(1, A + 1):
        a, v = make(), gpu.VectorIndex(vids, vx)
        gpu.alloc_fail_nth(n)
        err = None
        try:
            call(a, v)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None and err.code == gpu.E_NOMEM, f"{form} n={n}/{A}: {err}"
        check(call(a, v))
        a.close(); v.close()
    print(f"alloc-failure sweep search_ids {form}: A = {A} allocations, every one failed once: FREDDY_E_NOMEM, then the expected lists")
