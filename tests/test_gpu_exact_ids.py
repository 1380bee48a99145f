"""-m gpu: exact kNN and the exact kNN-join by row id (freddy_gpu_exact_search_ids / freddy_gpu_exact_join_ids) and option
exact_resolve: the queries are rows of the handle gathered on the device, the id set is resolved on the device (csrc/resolve.h).
Every list is held to the oracle's exact_knn over the set (as tests/test_gpu_exact_join.py::_expect does) and compared bit for bit
with the existing entry point fed the host-gathered rows, which resolves its set on the host.  The handle's profile names the
kernels that ran, so a case that silently takes another path fails."""
import ctypes as C

import numpy as np
import pytest

import exact_ids_inputs as ei
import util

pytestmark = pytest.mark.gpu

TO, POS = ei.TABLE_ORDER, ei.POSITIONAL
RESOLVE = {"resolve_mark", "resolve_scan", "resolve_place"}
JOIN_KERNELS = {"exact_join_gather", "exact_join_prep", "exact_join_sample", "exact_join_threshold", "exact_join_filter", "exact_join_refine"}
ALL_EXACT = {"exact_scan", "exact_merge"}
UNPIN = "unpin it and pin again"


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _table(d, N):
    x = util.shape_corpus(N, d).numpy().astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]              # duplicate rows: equal similarities, ties by id
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    return x, ids


@pytest.fixture(scope="module")
def main(gpu):
    """20 000 x 300 and 9 000 known targets among duplicates and unknown ids: the filter + refine path of the join."""
    x, ids = _table(ei.JOIN_D, ei.JOIN_N)
    targets = ei.join_targets(ids, ei.JOIN_KNOWN)
    assert ei.rows_of_ids(ids, targets).size == ei.JOIN_KNOWN
    idx = gpu.VectorIndex(ids, x)
    yield {"x": x, "ids": ids, "targets": targets, "idx": idx}
    idx.close()


def _profiled(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _bits_equal(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "ids differ")
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (what, "similarity bits differ")


def _fillers(gi, gs, what):
    assert (gi == -1).all() and np.isneginf(gs).all(), what


def _check_by_id(oracle, x, ids, q, rule, k, sset, got, host_call, what):
    """got = (sel, lists, sims) of a call by id: sel is the id rule's, every slot with a row equals the oracle and host_call(rows'
    vectors), every other slot is fillers."""
    sel, rows = ei.select(ids, q, rule)
    gq, gi, gs = got
    assert np.array_equal(gq, sel), (what, "out_query_ids")
    assert gi.shape == (sel.size, k) and gs.shape == (sel.size, k), what
    have = np.flatnonzero(rows >= 0)
    if have.size:
        qv = np.ascontiguousarray(x[rows[have]])
        _bits_equal((gi[have], gs[have]), host_call(qv), what)
        exp = [oracle.exact_knn(x, ids, v, k, sset) for v in qv]
        util.assert_exact_lists(gi[have], gs[have], exp, k, what)
    _fillers(gi[rows < 0], gs[rows < 0], what)


# ---- the join ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [TO, POS])
@pytest.mark.parametrize("Q", ei.JOIN_Q)
def test_join_ids_filter_and_refine(gpu, oracle, main, Q, rule):
    x, ids, targets, idx = main["x"], main["ids"], main["targets"], main["idx"]
    q = ei.query_ids(ids, Q, seed=Q)
    got, names = _profiled(idx, lambda: idx.exact_join_ids(q, 5, targets, rule=rule))
    st = idx.last_join_stats()
    assert names == JOIN_KERNELS | RESOLVE | ({"query_gather"} if Q > 1 else set()), sorted(names)
    assert st["filter_queries"] == Q and st["redone_queries"] == 0 and Q * 5 <= st["candidates"], st
    _check_by_id(oracle, x, ids, q, rule, 5, targets, got, lambda qv: idx.join(qv, 5, targets), f"join Q={Q} rule={rule}")
    assert idx.last_join_stats()["filter_queries"] == Q            # (the plain call reports the same way)
    assert idx.bound_violations() == 0


def test_join_ids_positional_with_unknown_and_repeated_ids(gpu, oracle, main):
    x, ids, targets, idx = main["x"], main["ids"], main["targets"], main["idx"]
    q = ei.query_ids(ids, 40, seed=3)
    q[[0, 7, 39]] = [4, -9, 10**8]          # unknown: first, middle, last slot
    q[11] = q[12] = q[30]                    # one id three times
    for k in (5, 32):
        got = idx.exact_join_ids(q, k, targets, rule=POS)
        assert idx.last_join_stats()["filter_queries"] == 37
        _check_by_id(oracle, x, ids, q, POS, k, targets, got, lambda qv: idx.join(qv, k, targets), f"positional k={k}")
    assert np.array_equal(got[1][11], got[1][30]) and np.array_equal(got[1][12], got[1][30])


def test_join_ids_table_order_leaves_the_slots_beyond_q_alone(gpu, main):
    ids, targets, idx = main["ids"], main["targets"], main["idx"]
    q = np.concatenate([ei.query_ids(ids, 20, seed=8), [6, -1], ids[[5, 5, 9]]]).astype(np.int32)
    sel, rows = ei.select(ids, q, TO)
    n, k = q.size, 5
    oq, oi, os_ = np.full(n, -77, np.int32), np.full((n, k), -77, np.int32), np.full((n, k), -77.0, np.float32)
    nq = C.c_int32(-9)
    P = gpu._p
    rc = idx.lib.freddy_gpu_exact_join_ids(idx.h, P(q), n, TO, k, P(targets), targets.size, P(oq), C.byref(nq), P(oi), P(os_))
    assert rc == 0 and nq.value == sel.size < n
    assert np.array_equal(oq[:sel.size], sel) and (oq[sel.size:] == -77).all()
    assert (oi[sel.size:] == -77).all() and (os_[sel.size:] == -77.0).all() and (oi[:sel.size] != -77).all()
    ref = idx.join(main["x"][rows], k, targets)
    _bits_equal((oi[:sel.size], os_[:sel.size]), ref, "table order")


# ---- the search ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("Q", [1, 33])
def test_search_ids_whole_table_and_subset(gpu, oracle, main, Q, k):
    """k = 5: the whole table through filter + refine (no bitmap: nothing of the resolve runs); k = 33: all-exact.  The subset always
    takes the all-exact kernels behind the device resolve."""
    x, ids, idx = main["x"], main["ids"], main["idx"]
    sub = main["targets"][:3000]
    q = ei.query_ids(ids, Q, seed=100 + Q)
    got, names = _profiled(idx, lambda: idx.exact_search_ids(q, k, rule=POS))
    assert not (names & RESOLVE) and (("exact_scan" in names) == (k > 32)), sorted(names)
    _check_by_id(oracle, x, ids, q, POS, k, None, got, lambda qv: idx.search(qv, k), f"whole table Q={Q} k={k}")
    got, names = _profiled(idx, lambda: idx.exact_search_ids(q, k, subset_ids=sub, rule=TO))
    assert names == ALL_EXACT | RESOLVE | ({"query_gather"} if Q > 1 else set()), sorted(names)
    _check_by_id(oracle, x, ids, q, TO, k, sub, got, lambda qv: idx.search(qv, k, subset_ids=sub), f"subset Q={Q} k={k}")


def test_search_ids_passes_of_k_above_1024_and_k_larger_than_the_set(gpu, oracle):
    x, ids = _table(300, 3000)
    idx = gpu.VectorIndex(ids, x)
    q = ei.query_ids(ids, 3, seed=4)
    got = idx.exact_search_ids(q, 1025, rule=POS)
    _check_by_id(oracle, x, ids, q, POS, 1025, None, got, lambda qv: idx.search(qv, 1025), "k=1025 over 3000 rows")
    sub = np.concatenate([ids[100:1400], ids[200:300], [2, -4]]).astype(np.int32)       # 1 300 rows: two passes, the second short
    got = idx.exact_search_ids(q, 1500, subset_ids=sub, rule=POS)
    _check_by_id(oracle, x, ids, q, POS, 1500, sub, got, lambda qv: idx.search(qv, 1500, subset_ids=sub), "k=1500 over 1300 rows")
    assert (got[1][:, 1300:] == -1).all() and (got[1][:, :1300] >= 0).all()
    few = ids[[7, 7, 900]]
    got = idx.exact_join_ids(q, 5, few, rule=POS)                                       # k larger than the set: fillers
    _check_by_id(oracle, x, ids, q, POS, 5, few, got, lambda qv: idx.join(qv, 5, few), "two targets, k=5")
    assert (got[1][:, 2:] == -1).all() and np.isneginf(got[2][:, 2:]).all()
    idx.close()


def test_all_exact_shape(gpu, oracle):
    """d = 30: no filter for this shape -- join and subset search by id through the all-exact kernels, resolve_block 8."""
    N, d = 9001, 30
    x, ids = _table(d, N)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("resolve_block", 8)
    targets = ei.join_targets(ids, 8500)
    for Q in (1, 33):
        q = ei.query_ids(ids, Q, seed=Q)
        got, names = _profiled(idx, lambda: idx.exact_join_ids(q, 5, targets))
        assert names == ALL_EXACT | RESOLVE | ({"query_gather"} if Q > 1 else set()), sorted(names)
        assert idx.last_join_stats() == {"filter_queries": 0, "candidates": 0, "redone_queries": 0}
        _check_by_id(oracle, x, ids, q, TO, 5, targets, got, lambda qv: idx.join(qv, 5, targets), f"d=30 Q={Q}")
    idx.close()


# ---- redo, non-finite rows, and the call after them -----------------------------------------------------------------------------------
def test_overflow_redo_and_the_next_call(gpu, oracle):
    """tests/test_gpu_exact_join.py::test_candidate_overflow_is_redone_all_exact by id: the query row equal to 10 000 target rows
    overflows its candidate buffer and is answered again all-exact, its row gathered again from the table (the filter's copy of the
    queries and the workspace it lay in are reused by then); the set stays resident through both.  Then the next call."""
    N, d = 20000, 300
    x, ids = _table(d, N)
    x[5000:15000] = x[4999]
    targets = np.concatenate([ids[4000:16000], np.array([4, -7], np.int32)])
    q = np.concatenate([ei.query_ids(ids[:3000], 69, seed=6), ids[4999:5000]]).astype(np.int32)
    q[[11, 69]] = q[[69, 11]]
    idx = gpu.VectorIndex(ids, x)
    got, names = _profiled(idx, lambda: idx.exact_join_ids(q, 5, targets, rule=POS))
    st = idx.last_join_stats()
    assert JOIN_KERNELS | RESOLVE | {"exact_scan", "query_gather"} <= names, sorted(names)
    assert st["filter_queries"] == 70 and 1 <= st["redone_queries"] < 70, st
    _check_by_id(oracle, x, ids, q, POS, 5, targets, got, lambda qv: idx.join(qv, 5, targets), "overflow by id")
    t2 = ids[:9000]
    q2 = ei.query_ids(ids, 33, seed=9)
    got = idx.exact_join_ids(q2, 5, t2)
    assert idx.last_join_stats()["redone_queries"] == 0
    _check_by_id(oracle, x, ids, q2, TO, 5, t2, got, lambda qv: idx.join(qv, 5, t2), "the call after the redo")
    assert idx.bound_violations() == 0
    idx.close()


def test_non_finite_query(gpu, oracle):
    """By id: a table with a non-finite row has no filter, so the row is answered -- among healthy ones -- by the all-exact kernels,
    as the plain call answers its vector.  With host queries and exact_resolve = 1 the filter does run over the resident set, finds
    the NaN query and the call falls back all-exact over the same resident rows: the lists of exact_resolve = 0, bit for bit."""
    N, d = 12000, 32
    x, ids = _table(d, N)
    idx = gpu.VectorIndex(ids, x)
    targets = ids[1000:10500]
    qs = x[:40].copy()
    qs[17, 3] = np.nan
    idx.set_option("exact_filter", 1)
    ref, names0 = _profiled(idx, lambda: idx.join(qs, 5, targets))
    idx.set_option("exact_resolve", 1)
    got, names1 = _profiled(idx, lambda: idx.join(qs, 5, targets))
    assert names1 == names0 | RESOLVE and "exact_join_prep" in names1 and "exact_scan" in names1, (sorted(names0), sorted(names1))
    _bits_equal(got, ref, "NaN query, exact_resolve=1")
    _bits_equal(idx.join(qs[:16], 5, targets), _with_option(idx, "exact_resolve", 0, lambda: idx.join(qs[:16], 5, targets)), "the call after the fall-back")
    idx.close()
    bad = x.copy()
    bad[77, 5] = np.inf
    idx = gpu.VectorIndex(ids, bad)
    q = np.concatenate([ids[70:80], ids[5000:5010]]).astype(np.int32)
    got, names = _profiled(idx, lambda: idx.exact_join_ids(q, 5, targets, rule=POS))
    assert names == ALL_EXACT | RESOLVE | {"query_gather"}, sorted(names)
    _sel, rows = ei.select(ids, q, POS)
    _bits_equal(got[1:], idx.join(bad[rows], 5, targets), "non-finite row by id")
    got2 = idx.exact_join_ids(q[:3], 5, targets, rule=POS)
    _bits_equal(got2[1:], (got[1][:3], got[2][:3]), "the call after it")
    idx.close()


def _with_option(idx, name, value, call):
    idx.set_option(name, value)
    return call()


# ---- empty work -----------------------------------------------------------------------------------------------------------------------
def test_empty_sets_and_unknown_ids(gpu, main):
    ids, targets, idx = main["ids"], main["targets"], main["idx"]
    q = ei.query_ids(ids, 9, seed=1)
    for t, what in ((np.zeros(0, np.int32), "n_targets = 0"), (np.array([4, -7, 10**8], np.int32), "only unknown targets")):
        gq, gi, gs = idx.exact_join_ids(q, 5, t, rule=POS)
        assert np.array_equal(gq, q), what
        _fillers(gi, gs, what)
        _bits_equal((gi, gs), idx.join(main["x"][ei.select(ids, q, POS)[1]], 5, t), what)
        gq, gi, gs = idx.exact_search_ids(q, 5, subset_ids=t if t.size else np.array([-1], np.int32), rule=POS)
        _fillers(gi, gs, what + " (search)")
    unknown = np.array([4, -7, 10**8, 6], np.int32)
    for call in (lambda r: idx.exact_join_ids(unknown, 5, targets, rule=r), lambda r: idx.exact_search_ids(unknown, 5, rule=r),
                 lambda r: idx.exact_search_ids(unknown, 5, subset_ids=targets, rule=r)):
        for rule in (TO, POS):
            (gq, gi, gs), names = _profiled(idx, lambda: call(rule))
            assert names == set(), ("only unknown query ids launch nothing", sorted(names))
            assert gq.size == (0 if rule == TO else 4)
            _fillers(gi, gs, "unknown query ids")
    assert idx.exact_join_ids(np.zeros(0, np.int32), 5, targets)[0].size == 0


# ---- option exact_resolve on the existing entry points ----------------------------------------------------------------------------------
def test_exact_resolve_option_changes_no_result(gpu, main):
    x, ids, targets, idx = main["x"], main["ids"], main["targets"], main["idx"]
    qs = np.ascontiguousarray(x[::150][:70])
    sub = targets[:3000]
    triples = np.stack([ids[10:16], ids[200:206], ids[4000:4006]], axis=1).astype(np.int32)
    triples[2, 1] = 4                                  # an unknown input id
    calls = {
        "join, filter + refine": lambda: idx.join(qs, 5, targets),
        "join, one query": lambda: idx.join(qs[:1], 32, targets),
        "join, k = 33": lambda: idx.join(qs[:9], 33, targets),
        "join, empty": lambda: idx.join(qs[:3], 5, np.zeros(0, np.int32)),
        "search, subset": lambda: idx.search(qs[:33], 5, subset_ids=sub),
        "search, subset, k = 1025": lambda: idx.search(qs[:3], 1025, subset_ids=sub),
        "3cosadd, subset": lambda: idx.analogy(triples, 3, "3cosadd", subset_ids=sub),
        "3cosmul, subset": lambda: idx.analogy(triples, 3, "3cosmul", subset_ids=sub),
        "pair direction, subset": lambda: idx.analogy(triples, 2, "pair_direction", subset_ids=sub),
        "analogy, unknown subset": lambda: idx.analogy(triples, 2, "3cosadd", subset_ids=np.array([4, -7], np.int32)),
    }
    try:
        for what, call in calls.items():
            idx.set_option("exact_resolve", 0)
            ref, names0 = _profiled(idx, call)
            assert not (names0 & RESOLVE), (what, sorted(names0))
            idx.set_option("exact_resolve", 1)
            got, names1 = _profiled(idx, call)
            assert names1 - names0 == (RESOLVE if "empty" not in what else set()), (what, sorted(names0), sorted(names1))
            assert names0 <= names1, what
            assert np.array_equal(got[0], ref[0]), what
            assert got[1].tobytes() == ref[1].tobytes(), what
    finally:
        idx.set_option("exact_resolve", 0)


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
def test_after_update_remove_append(gpu):
    """After each mutation of the handle a call by id answers as a fresh pin of the new table does (filter forced on: d = 32)."""
    N, d = 9001, 32
    x, ids = _table(d, N + 500)
    rng = np.random.default_rng(3)
    cur_x, cur_ids = x[:N].copy(), ids[:N].copy()
    idx = gpu.VectorIndex(cur_ids, cur_x)
    idx.set_option("exact_filter", 1)
    idx.set_option("resolve_block", 8)

    def check(what):
        q = np.concatenate([ei.query_ids(cur_ids, 33, seed=len(what)), [4]]).astype(np.int32)
        t = np.concatenate([cur_ids[rng.choice(cur_ids.size, 6000, replace=False)], ids[:50], [-3]]).astype(np.int32)
        fresh = gpu.VectorIndex(cur_ids, cur_x)
        fresh.set_option("exact_filter", 1)
        for rule in (TO, POS):
            got, names = _profiled(idx, lambda: idx.exact_join_ids(q, 5, t, rule=rule))
            assert "exact_join_filter" in names and RESOLVE <= names, (what, sorted(names))
            exp = fresh.exact_join_ids(q, 5, t, rule=rule)
            assert np.array_equal(got[0], exp[0]), what
            _bits_equal(got[1:], exp[1:], what)
            sel, rows = ei.select(cur_ids, q, rule)
            have = rows >= 0
            _bits_equal((got[1][have], got[2][have]), fresh.join(cur_x[rows[have]], 5, t), what + " (host rows)")
        fresh.close()

    check("as pinned")
    up = cur_ids[rng.choice(N, 300, replace=False)]
    new_rows = x[N:N + 300] * np.float32(0.5)
    idx.update_rows(up, vectors=new_rows)
    cur_x[np.searchsorted(cur_ids, up)] = new_rows
    check("after update_rows")
    gone = cur_ids[rng.choice(N, 1200, replace=False)]
    assert idx.remove_rows(gone) == 1200
    keep = ~np.isin(cur_ids, gone)
    cur_x, cur_ids = cur_x[keep], cur_ids[keep]
    check("after remove_rows")
    idx.append_rows(ids[N:N + 500], vectors=x[N:N + 500])
    cur_x, cur_ids = np.concatenate([cur_x, x[N:N + 500]]), np.concatenate([cur_ids, ids[N:N + 500]])
    check("after append_rows")
    assert idx.bound_violations() == 0
    idx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, idx_h):
    """(search_ids, join_ids) as raw calls with overridable arguments -> rc; the outputs start as -77 / -9."""
    lib, P = gpu.load(), gpu._p
    st = {"q": np.array([4, 6, 8], np.int32), "oq": np.full(3, -77, np.int32), "oi": np.full((3, 5), -77, np.int32),
          "os": np.full((3, 5), -77.0, np.float32), "nq": C.c_int32(-9), "set": np.array([5, 7], np.int32)}   # (even ids have no row in the tables of this file)

    def call(fn, h=idx_h, q=True, n=3, rule=TO, k=5, s=True, ns=2, oq=True, nq=True, oi=True, os_=True):
        return fn(h, P(st["q"]) if q else None, n, rule, k, P(st["set"]) if s else None, ns, P(st["oq"]) if oq else None,
                  C.byref(st["nq"]) if nq else None, P(st["oi"]) if oi else None, P(st["os"]) if os_ else None)
    return st, [lambda **kw: call(lib.freddy_gpu_exact_search_ids, **kw), lambda **kw: call(lib.freddy_gpu_exact_join_ids, **kw)]


def test_refusals_in_the_documented_order(gpu, main):
    idx = main["idx"]
    pq_t = util.shape_pq_tables(32, 8, 16, 600)
    other = gpu.PQIndex(pq_t["codebook"], pq_t["ids"], pq_t["codes"])
    st, calls = _raw(gpu, idx.h)
    lib = gpu.load()
    idx.profile_enable(True)
    for f in calls:
        # the front checks, each with every later refusal present as well
        assert f(h=None, n=-1, rule=7, k=0) == -1 and "NULL index" in lib.freddy_gpu_last_error().decode()
        assert f(n=-1, rule=7, k=0, h=other.h) == -1 and "n_ids" in lib.freddy_gpu_last_error().decode()
        assert f(rule=7, k=0, h=other.h) == -1 and "id_rule" in lib.freddy_gpu_last_error().decode()
        assert f(nq=False, k=0, h=other.h) == -1 and "n_queries" in lib.freddy_gpu_last_error().decode()
        for kw in ({"q": False}, {"oq": False}, {"oi": False}, {"os_": False}):
            assert f(k=0, h=other.h, **kw) == -1 and "NULL buffer" in lib.freddy_gpu_last_error().decode(), kw
        # what the entry point underneath refuses, before the handle's kind is looked at
        assert f(k=0, h=other.h) == -1 and f(k=-3, h=other.h) == -1
        assert f(ns=-1, h=other.h) == -1
        assert f(s=False, ns=2, h=other.h) == -1
        assert f(k=4097, h=other.h) == -5 and "4096" in lib.freddy_gpu_last_error().decode()
        assert f(k=4097, ns=-1, h=other.h) == -1                         # (sizes before the limit)
        # the kind
        assert f(h=other.h) == -4
        assert st["nq"].value == -9 and (st["oq"] == -77).all() and (st["oi"] == -77).all() and (st["os"] == -77.0).all()
        # and what is not refused
        assert f(k=4096, ns=0, s=False) == 0 and st["nq"].value == 0      # (no id has a row: nothing is searched, nothing written)
        st["nq"].value = -9
        assert f(n=0, q=False, oq=False, oi=False, os_=False) == 0 and st["nq"].value == 0
        st["nq"].value = -9
    assert idx.profile_read() == {}, "a refused call launched something"
    idx.profile_enable(False)
    other.close()


def test_a_poisoned_handle_is_refused(gpu):
    """As tests/test_gpu_query_ids.py poisons one: an allocation of update_rows fails after its first write in place."""
    x, ids = _table(32, 600)
    make = lambda: gpu.VectorIndex(ids, x)
    mutate = lambda h: h.update_rows(ids[:40], vectors=x[40:80])
    lib, P = gpu.load(), gpu._p
    one_q, o1, o2 = x[:1], np.empty((1, 1), np.int32), np.empty((1, 1), np.float32)
    ref = make()
    c0 = gpu.alloc_stats().calls
    mutate(ref)
    A = gpu.alloc_stats().calls - c0
    ref.close()
    bad = None
    for n in range(A, 0, -1):
        h = make()
        gpu.alloc_fail_nth(n)
        try:
            mutate(h)
        except gpu.FreddyGpuError as e:
            assert e.code == gpu.E_NOMEM, e
        finally:
            gpu.alloc_fail_nth(0)
        rc = lib.freddy_gpu_exact_search(h.h, P(one_q), 1, 0, None, 0, P(o1), P(o2))
        assert rc in (-1, -2), rc
        if rc == -2:
            bad = h
            break
        h.close()
    assert bad is not None, f"none of the {A} allocations of update_rows, failed, poisons the handle"
    st, calls = _raw(gpu, bad.h)
    st["q"][:] = ids[:3]
    bad.profile_enable(True)
    c0 = gpu.alloc_stats().calls
    for f in calls:
        assert f(k=0) == -1                                               # the scalar checks still come first
        assert f() == -2 and UNPIN in lib.freddy_gpu_last_error().decode()
        assert st["nq"].value == -9 and (st["oq"] == -77).all() and (st["oi"] == -77).all()
    out, n = np.full(3, -7, np.int32), C.c_int64(-9)
    assert lib.freddy_gpu_debug_resolve_ids(bad.h, P(st["q"]), 3, P(out), C.byref(n)) == -2 and n.value == -9
    assert gpu.alloc_stats().calls == c0 and bad.profile_read() == {}
    bad.close()


# ---- allocation failures --------------------------------------------------------------------------------------------------------------
def test_every_allocation_of_the_new_calls_fails_once(gpu):
    """As tests/test_gpu_alloc_failures.py walks a call: its allocations are counted on a fresh handle (A, which must reach the
    floor read off the code), then for every n in 1 .. A a fresh handle is pinned and the n-th allocation fails: FREDDY_E_NOMEM,
    exactly one failure, and the handle answers the same call -- and the plain ones -- as the reference handle did.
    Floors: the resolve takes 5 device buffers and the pinned word (6); a subset search adds the two subset buffers and four of the
    scan (12); the filtered join adds at least eight workspace buffers of its own to the resolve's (14)."""
    N, d = 9001, 32
    x, ids = _table(d, N)
    q = np.concatenate([ei.query_ids(ids, 33, seed=2), [4]]).astype(np.int32)
    t = ei.join_targets(ids, 8200)
    sub = t[:2000]

    def pin():
        h = gpu.VectorIndex(ids, x)
        h.set_option("exact_filter", 1)
        return h
    scenarios = [("debug_resolve_ids", 6, lambda h: (h.debug_resolve_ids(t),)),
                 ("exact_search_ids, subset", 12, lambda h: h.exact_search_ids(q, 5, subset_ids=sub, rule=POS)),
                 ("exact_join_ids", 14, lambda h: h.exact_join_ids(q, 5, t, rule=POS))]
    for what, floor, call in scenarios:
        ref = pin()
        c0 = gpu.alloc_stats().calls
        expected = call(ref)
        A = gpu.alloc_stats().calls - c0
        plain = ref.join(x[:20], 5, t)
        ref.close()
        assert A >= floor, (what, A)
        for n in range(1, A + 1):
            h = pin()
            f0 = gpu.alloc_stats().failed
            gpu.alloc_fail_nth(n)
            try:
                with pytest.raises(gpu.FreddyGpuError) as e:
                    call(h)
            finally:
                gpu.alloc_fail_nth(0)
            assert e.value.code == gpu.E_NOMEM and len(str(e.value)) > 20, (what, n, str(e.value))
            assert gpu.alloc_stats().failed - f0 == 1, (what, n)
            got = call(h)                                                   # the handle is as it was: the same call answers
            for a, b in zip(got, expected):
                assert a.tobytes() == b.tobytes(), (what, n)
            _bits_equal(h.join(x[:20], 5, t), plain, (what, n, "the plain join afterwards"))
            assert h.bound_violations() == 0
            h.close()
