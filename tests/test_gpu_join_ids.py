"""-m gpu: the kNN-join by row id (include/freddy_gpu.h: freddy_gpu_knn_join_ids; the binding IVPQIndex.knn_join_ids).  The queries are rows
of a pinned vector table -- or of the ivpq handle's own vectors -- selected by the id rule on the host and gathered on the device by the
kernel that computes their sub-distances (join_kernels.h sub_dist_rows_kernel; option join_front_gather = 0: query_gather_kernel, then
sub_dist_kernel).

Expected lists and iteration counts come from the oracle alone (tests/join_ids_inputs.py; tests/test_join_ids_inputs_cpu.py shows what
the inputs exercise), and every result is also compared bit for bit with knn_join over the same rows' vectors."""
import ctypes as C

import numpy as np
import pytest

import join_ids_inputs as ji
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND, E_LIMIT = "freddy_gpu error -1", "freddy_gpu error -4", "freddy_gpu error -5"
TO, POS = ji.TABLE_ORDER, ji.POSITIONAL
FRONTS = {1: "join_front_rows", 0: "query_gather"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def handles(gpu):
    """every shape's handles, pinned once: the ivpq index and the three vector tables"""
    out = {}
    for shape in ji.SHAPES:
        h = {"ivpq": gpu.IVPQIndex(*ji.pin_args(ji.tables(shape))), "x": np.asarray(ji.tables(shape)["vectors"], np.float32)}
        for which in ("same", "more", "fewer"):
            h[which] = gpu.VectorIndex(*ji.vec_table(shape, which))
        out[shape] = h
    yield out
    for h in out.values():
        for n in ("ivpq", "same", "more", "fewer"):
            h[n].close()


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _bits_equal(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what


def _join_ids(ivpq, vecs, ids, case, method, use_tl=True, rule=POS):
    k, alpha, pvf, T, conf = case
    return ivpq.knn_join_ids(vecs, ids, k, ji.targets(T), alpha, pvf, method, id_rule=rule, use_target_lists=use_tl, confidence=conf)


def _join(ivpq, qs, case, method, use_tl=True):
    k, alpha, pvf, T, conf = case
    return ivpq.knn_join(qs, k, ji.targets(T), alpha, pvf, method, use_target_lists=use_tl, confidence=conf)


# ---- shapes x methods x target lists: both vector sources, both fronts -----------------------------------------------------------
@pytest.mark.parametrize("use_tl", [True, False])
@pytest.mark.parametrize("method", ji.METHODS)
@pytest.mark.parametrize("shape", ji.SHAPES)
def test_lists_and_iterations(handles, oracle, shape, method, use_tl):
    h = handles[shape]
    ivpq, qids, qs = h["ivpq"], ji.query_ids(), h["x"][ji.query_rows()]
    for case in ji.CASES:
        exp, eit = ji.expected(oracle, shape, method, case, use_tl)
        fi, fd, fit = _join(ivpq, qs, case, method, use_tl)                          # the float entry point over the same rows
        for vecs in (h["same"], None):
            for gather in (1, 0):
                what = f"{shape} method={method} tl={use_tl} case={case} own={vecs is None} join_front_gather={gather}"
                ivpq.set_option("join_front_gather", gather)
                try:
                    (gq, gi, gd, git), names = _profiled(ivpq, lambda: _join_ids(ivpq, vecs, qids, case, method, use_tl))
                finally:
                    ivpq.set_option("join_front_gather", 1)
                assert np.array_equal(gq, qids) and git == eit == fit, (what, git, eit, fit)
                util.assert_same_lists(gi, gd, exp, what)
                _bits_equal((gi, gd), (fi, fd), what)
                assert names == {FRONTS[gather]}, (what, sorted(names))
                assert ivpq.last_track()["iterations"] == eit, what


# ---- a vector table with more ids than the ivpq table, and one that lacks some -----------------------------------------------------
@pytest.mark.parametrize("shape", ji.SHAPES)
def test_other_vector_tables(handles, oracle, shape):
    h = handles[shape]
    ivpq, table, case = h["ivpq"], ji.oracle_table(oracle, shape), ji.CASES[0]
    k, alpha, pvf, T, conf = case
    # more: rows the ivpq table does not hold are queries like any other
    vids, vx = ji.vec_table(shape, "more")
    ids = np.concatenate([ji.query_ids()[:6], vids[-5:], [vids[ji.N]]]).astype(np.int32)
    sel, rows = ji.model(vids, ids, POS)
    assert (rows >= 0).all() and (rows >= ji.N).sum() == 6
    for method in ji.METHODS:
        exp, eit = oracle.ivpq_search_in(table, vx[rows], k, ji.targets(T), alpha, pvf, method, confidence=conf)
        gq, gi, gd, git = _join_ids(ivpq, h["more"], ids, case, method)
        assert np.array_equal(gq, ids) and git == eit
        util.assert_same_lists(gi, gd, exp, f"{shape} more method={method}")
    # fewer: most ids have no row there -- fillers in their positional slots, gone in table order
    vids, vx = ji.vec_table(shape, "fewer")
    ids = ji.query_ids()
    for rule in (POS, TO):
        sel, rows = ji.model(vids, ids, rule)
        live = rows >= 0
        exp, eit = oracle.ivpq_search_in(table, vx[rows[live]], k, ji.targets(T), alpha, pvf, 1, confidence=conf)
        gq, gi, gd, git = _join_ids(ivpq, h["fewer"], ids, case, 1, rule=rule)
        assert np.array_equal(gq, sel) and git == eit, rule
        util.assert_same_lists(gi[live], gd[live], exp, f"{shape} fewer rule={rule}")
        assert (gi[~live] == -1).all() and (gd[~live] == ji.FILLER).all()
        fi, fd, fit = _join(ivpq, vx[rows[live]], case, 1)
        _bits_equal((gi[live], gd[live]), (fi, fd), f"{shape} fewer rule={rule}")


# ---- POSITIONAL with unknown, negative and repeated ids; TABLE_ORDER ----------------------------------------------------------------
@pytest.mark.parametrize("shape", ji.SHAPES)
def test_positional_slots(handles, oracle, shape):
    h = handles[shape]
    ivpq = h["ivpq"]
    noisy = ji.noisy_positional(ji.query_ids())
    live = np.array([1, 2, 4, 5, 7])
    dead = np.array([0, 3, 6, 8])
    sub_rows = ji.query_rows()[list(ji.SUB_BATCH)]
    for case in ji.CASES:
        for method in ji.METHODS:
            whole, _ = ji.expected(oracle, shape, method, case)
            part, pit = ji.expected(oracle, shape, method, case, rows=sub_rows)      # ONE join over the compacted batch
            for vecs in (h["same"], None, h["more"]):
                what = f"{shape} positional method={method} case={case}"
                gq, gi, gd, git = _join_ids(ivpq, vecs, noisy, case, method)
                assert np.array_equal(gq, noisy) and gi.shape == (noisy.size, case[0]) and git == pit, what
                util.assert_same_lists(gi[live], gd[live], part, what)
                util.assert_same_lists(gi[live], gd[live], whole[list(ji.SUB_BATCH)], what + ": the batch without them")
                assert (gi[dead] == -1).all() and (gd[dead] == ji.FILLER).all(), what


def test_table_order_leaves_the_slots_beyond_q_alone(gpu, handles, oracle):
    """The C call itself (the binding cuts its arrays to n_queries): the buffers hold n_ids slots, TABLE_ORDER fills the first Q."""
    shape = ji.SHAPES[2]
    h = handles[shape]
    ivpq, vec = h["ivpq"], h["same"]
    noisy = ji.noisy_positional(ji.query_ids())
    k, alpha, pvf, T, conf = case = ji.CASES[1]
    sel, rows = ji.model(ji.vec_table(shape, "same")[0], noisy, TO)
    n, tg = noisy.size, ji.targets(T)
    oq, oi, od = np.full(n, -77, np.int32), np.full((n, k), -77, np.int32), np.full((n, k), -77.0, np.float32)
    nq, it = C.c_int32(-1), C.c_int32(-1)
    P = gpu._p
    for v in (vec.h, None):
        oq[:], oi[:], od[:] = -77, -77, -77.0
        gpu._check(ivpq.lib.freddy_gpu_knn_join_ids(ivpq.h, v, P(noisy), n, TO, k, P(tg), tg.size, alpha, pvf, 0, 1, C.c_float(conf), 10000000, P(oq),
                                                    C.byref(nq), P(oi), P(od), C.byref(it)))
        Q = nq.value
        assert Q == sel.size == 4 < n and np.array_equal(oq[:Q], sel) and (np.diff(sel) > 0).all()
        exp, eit = ji.expected(oracle, shape, 0, case, rows=rows)
        assert it.value == eit
        util.assert_same_lists(oi[:Q], od[:Q], exp, "the first Q slots")
        assert (oq[Q:] == -77).all() and (oi[Q:] == -77).all() and (od[Q:] == -77.0).all()


def test_only_unknown_ids_launch_nothing(handles):
    h = handles[ji.SHAPES[0]]
    ivpq = h["ivpq"]
    unknown = np.array([0, -3, ji.N + 1, 2 ** 30], np.int32)
    case = ji.CASES[0]
    for vecs in (h["same"], None):
        (gq, gi, gd, git), names = _profiled(ivpq, lambda: _join_ids(ivpq, vecs, unknown, case, 0, rule=TO))
        assert gq.size == 0 and gi.shape == (0, case[0]) and names == set() and git == 0
        (gq, gi, gd, git), names = _profiled(ivpq, lambda: _join_ids(ivpq, vecs, unknown, case, 0, rule=POS))
        assert np.array_equal(gq, unknown) and names == set() and git == 0
        assert (gi == -1).all() and (gd == ji.FILLER).all()
        (gq, gi, gd, git), names = _profiled(ivpq, lambda: _join_ids(ivpq, vecs, np.empty(0, np.int32), case, 0))
        assert gq.size == 0 and gi.shape == (0, case[0]) and names == set() and git == 0       # n_ids == 0 succeeds


# ---- the host heap, a mutation of the vector table, the target-list cache ----------------------------------------------------------
def test_host_traversal(gpu, oracle):
    shape = ji.SHAPES[2]
    ix = gpu.IVPQIndex(*ji.pin_args(ji.tables(shape)))
    ix.set_option("join_host_traversal", 1)
    try:
        for method in ji.METHODS:
            exp, eit = ji.expected(oracle, shape, method, ji.CASES[1])
            gq, gi, gd, git = _join_ids(ix, None, ji.query_ids(), ji.CASES[1], method)
            assert git == eit and ix.last_track()["host_traversals"] > 0
            util.assert_same_lists(gi, gd, exp, f"host traversal method={method}")
    finally:
        ix.close()


def test_after_update_rows_on_the_vector_handle(gpu, handles, oracle):
    shape = ji.SHAPES[1]
    ivpq = handles[shape]["ivpq"]
    vids, vx = ji.vec_table(shape, "same")
    vx = vx.copy()
    vec = gpu.VectorIndex(vids, vx)
    qids, case = ji.query_ids(), ji.CASES[0]
    k, alpha, pvf, T, conf = case
    try:
        before = _join_ids(ivpq, vec, qids, case, 1)
        new = -vx[ji.query_rows()[:7][::-1]]
        assert vec.update_rows(qids[:7], vectors=new) == 7
        vx[ji.query_rows()[:7]] = new
        exp, eit = oracle.ivpq_search_in(ji.oracle_table(oracle, shape), vx[ji.query_rows()], k, ji.targets(T), alpha, pvf, 1, confidence=conf)
        gq, gi, gd, git = _join_ids(ivpq, vec, qids, case, 1)
        assert git == eit
        util.assert_same_lists(gi, gd, exp, "after update_rows")
        fi, fd, fit = _join(ivpq, vx[ji.query_rows()], case, 1)
        _bits_equal((gi, gd), (fi, fd), "after update_rows: knn_join over the new vectors")
        assert not np.array_equal(gi[:7], before[1][:7])
        oi, od, oit = _join_ids(ivpq, None, qids, case, 1)[1:]                        # the ivpq handle's own vectors did not change
        _bits_equal((oi, od), before[1:3], "own vectors")
    finally:
        vec.close()


def test_a_repeated_target_array(gpu, oracle):
    """The previous call's target buckets serve a call with the same array, whichever of the two entry points made it."""
    shape = ji.SHAPES[0]
    ix = gpu.IVPQIndex(*ji.pin_args(ji.tables(shape)))
    vec = gpu.VectorIndex(*ji.vec_table(shape, "same"))
    qs = np.asarray(ji.tables(shape)["vectors"], np.float32)[ji.query_rows()]
    try:
        for first in ("float", "ids"):
            for case in (ji.CASES[0], ji.CASES[1]):                                   # (another target array in between: a miss)
                exp, eit = ji.expected(oracle, shape, 0, case)
                order = [lambda: _join(ix, qs, case, 0), lambda: _join_ids(ix, vec, ji.query_ids(), case, 0)[1:]]
                for call in (order if first == "float" else order[::-1]) * 2:
                    gi, gd, git = call()
                    assert git == eit
                    util.assert_same_lists(gi, gd, exp, f"repeated targets, {first} first, case={case}")
    finally:
        ix.close()
        vec.close()


# ---- refusals: the documented order, nothing launched, nothing written ---------------------------------------------------------------
def test_refusals(gpu, handles):
    shape = ji.SHAPES[2]
    h = handles[shape]
    ivpq, vec = h["ivpq"], h["same"]
    lib, P = ivpq.lib, gpu._p
    q, tg = np.array([1, 4, 7], np.int32), ji.targets(300)
    oq, oi, od = np.full(3, -77, np.int32), np.full((3, 5), -77, np.int32), np.full((3, 5), -77.0, np.float32)
    nq, it = C.c_int32(-9), C.c_int32(-9)
    other = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), util.shape_corpus(6000, 30).numpy()[:100])
    t = ji.tables(shape)
    bare = gpu.IVPQIndex(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], None, t["stats"])

    def call(a=ivpq.h, v=vec.h, ids=P(q), n=3, rule=0, k=5, tids=P(tg), nt=tg.size, alpha=1, pvf=3, method=0, oq_=P(oq), nq_=C.byref(nq), oi_=P(oi),
             od_=P(od)):
        return lib.freddy_gpu_knn_join_ids(a, v, ids, n, rule, k, tids, nt, alpha, pvf, method, 1, C.c_float(0.8), 10000000, oq_, nq_, oi_, od_, C.byref(it))

    table = [
        (dict(a=None), E_ARG, "NULL index"), (dict(n=-1), E_ARG, "n_ids=-1"), (dict(rule=2), E_ARG, "bad id_rule 2"),
        (dict(nq_=None), E_ARG, "NULL n_queries"), (dict(ids=None), E_ARG, "NULL buffer"), (dict(oq_=None), E_ARG, "NULL buffer"),
        (dict(oi_=None), E_ARG, "NULL buffer"), (dict(od_=None), E_ARG, "NULL buffer"),
        (dict(k=0), E_ARG, "bad sizes"), (dict(nt=-1), E_ARG, "bad sizes"), (dict(tids=None), E_ARG, "NULL target ids"),
        (dict(method=3), E_ARG, "Unknown computation method!"), (dict(k=4097), E_LIMIT, "k=4097"), (dict(k=100, pvf=82, method=2), E_LIMIT, "k\\*pvf=8200"),
        (dict(a=bare.h, method=1), E_ARG, "methods 1 and 2 need the vectors to be pinned"),
        (dict(a=vec.h), E_KIND, "wrong kind"), (dict(v=ivpq.h), E_KIND, "wrong kind"), (dict(a=vec.h, v=None), E_KIND, "wrong kind"),
        (dict(v=other.h), E_ARG, "vectors have 30 dimensions, the index has 300"),
        (dict(a=bare.h, v=None), E_ARG, "pinned without vectors"),
        # the order: the front checks before the join's, the join's before the kinds, the kinds before the shapes
        (dict(rule=5, k=0, a=vec.h), E_ARG, "bad id_rule 5"), (dict(k=0, a=vec.h), E_ARG, "bad sizes"), (dict(method=7, v=ivpq.h), E_ARG, "Unknown computation"),
        (dict(a=vec.h, v=other.h), E_KIND, "wrong kind"),
    ]
    try:
        for idx in (ivpq, bare):
            idx.profile_enable(True)
        c0 = gpu.alloc_stats().calls
        for kw, code, msg in table:
            with pytest.raises(gpu.FreddyGpuError, match=code + ".*" + msg):
                gpu._check(call(**kw))
            assert nq.value == -9 and it.value == -9, kw                              # nothing written
        assert gpu.alloc_stats().calls == c0, "a refused call allocated"
        for idx in (ivpq, bare):
            assert set(idx.profile_read()) == set(), "a refused call launched something"
            idx.profile_enable(False)
        assert (oq == -77).all() and (oi == -77).all() and (od == -77.0).all()
        assert call(n=0, ids=None, oq_=None, oi_=None, od_=None) == 0 and nq.value == 0 and it.value == 0     # n_ids == 0 succeeds
    finally:
        other.close()
        bare.close()


def test_a_handle_pinned_without_vectors_takes_a_vector_handle(gpu, handles, oracle):
    shape = ji.SHAPES[0]
    t = ji.tables(shape)
    bare = gpu.IVPQIndex(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], None, t["stats"])
    try:
        with pytest.raises(gpu.FreddyGpuError, match=E_ARG + ".*pinned without vectors"):
            _join_ids(bare, None, ji.query_ids(), ji.CASES[0], 0)
        for case in ji.CASES[:2]:
            exp, eit = ji.expected(oracle, shape, 0, case)
            gq, gi, gd, git = _join_ids(bare, handles[shape]["same"], ji.query_ids(), case, 0)
            assert git == eit
            util.assert_same_lists(gi, gd, exp, f"no own vectors, case={case}")
    finally:
        bare.close()
