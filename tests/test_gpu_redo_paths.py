"""-m gpu: the redo half of the exact filter + refine design.  Exact kNN, the exact analogies and the exact join answer a query
(a pass of 32 analogies) whose candidate buffer of 8 192 rows overflows, or whose columns are not finite, again on the all-exact
path; these tests make that happen at chosen places among healthy inputs and compare every list, ids and score bits, with
analogy_model / the oracle -- the redone ones, the ones beside them that must stay the filter's, and the lists of LATER calls on
the same handle, which read the verdict words, the arrival counter and the overflow flag the fallback left behind.

The inputs are tests/redo_inputs.py's: a 20 000 x 300 table in which 10 001 rows are equal.  WHICH passes and queries are redone
is asserted from what tests/test_redo_inputs_cpu.py proves about them (a hot input has more tied candidates than a buffer holds,
a healthy one keeps the copies 0.05 below its 32nd best score), never from a recorded run.  The handle's profile names the
kernels that ran, so a call that silently takes the other path fails."""
import numpy as np
import pytest

import redo_inputs as ri

pytestmark = pytest.mark.gpu

METHODS = ["3cosadd", "3cosmul"]
KS = (1, 5, 32)
FILTER, SCAN = {"exact_filter", "exact_refine"}, {"exact_scan", "exact_merge"}
AN_FILTER, AN_SCAN = {"analogy_filter", "analogy_refine"}, {"analogy_scan", "analogy_merge"}
JOIN_KERNELS = {"exact_join_gather", "exact_join_prep", "exact_join_sample", "exact_join_threshold", "exact_join_filter", "exact_join_refine"}
HOT_IN_PASS_1 = {32: ri.HOT_TRIPLES[0], 41: ri.HOT_TRIPLES[1], 63: ri.HOT_TRIPLES[2]}   # the first, one inside, the last of pass 1


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    """(the call's result, {kernel: launches})."""
    idx.profile_enable(True)
    out = call()
    prof = {name: v[0] for name, v in idx.profile_read().items()}
    idx.profile_enable(False)
    return out, prof


def _nan_as_one(a):
    """float bits with every NaN as one pattern (which NaN an invalid operation produces is the processor's choice)."""
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _same_analogies(got, exp, what):
    (gi, gs), (ei, es) = got, exp
    assert np.array_equal(gi, ei), (what, np.nonzero((gi != ei).any(1))[0][:8])
    assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)), (what, np.nonzero((gs.view(np.uint64) != es.view(np.uint64)).any(1))[0][:8])


def _same_lists(gi, gs, exp, k, what):
    """Every query's list against the oracle's entries (the first k of a list of 32)."""
    assert gi.shape[0] == len(exp)
    for qi, e in enumerate(exp):
        e = e[:k]
        assert gi[qi].tolist() == e["id"].tolist(), (what, qi)
        assert np.array_equal(_nan_as_one(gs[qi]), _nan_as_one(e["dist"])), (what, qi)


@pytest.fixture(scope="module")
def knn(oracle):
    """Expected lists of 32, computed once: the healthy queries' and the hot query's over the whole table."""
    x, ids = ri.table()
    return dict(healthy=[oracle.exact_knn(x, ids, q, ri.K_MAX) for q in ri.queries()], hot=oracle.exact_knn(x, ids, ri.hot_query(), ri.K_MAX))


def _knn_expected(knn, oracle, qs, at, bad):
    x, ids = ri.table()
    exp = list(knn["healthy"][:len(qs)])
    for i in at:
        exp[i] = knn["hot"] if bad is None else oracle.exact_knn(x, ids, qs[i], ri.K_MAX)
    return exp


# ---- a. / b. / c. analogies ------------------------------------------------------------------------------------------------
def _analogy_call(idx, call, k, method):
    got, prof = _profiled(idx, lambda: idx.analogy(call["triples"], k=k, method=method))
    _same_analogies(got, ri.analogy_expected(call, k, method), (method, k))
    unknown = np.setdiff1d(np.arange(call["triples"].shape[0]), call["live"])
    assert (got[0][unknown] == -1).all() and np.isneginf(got[1][unknown]).all()
    return got, prof, idx.last_analogy_stats()


@pytest.mark.parametrize("method", METHODS)
def test_analogy_one_pass_of_three_is_redone(gpu, method):
    """70 live triples among 73 (unknown ids at caller positions 2, 35 and 71), hot ones only in pass 1 of the LIVE numbering:
    that pass alone is computed again, by one scan launch that writes into the middle of the device lists, and its candidates
    are not counted.  Then a healthy call on the same handle: nothing redone, no scan."""
    x, ids = ri.table()
    call = ri.analogy_call(HOT_IN_PASS_1)
    idx = gpu.VectorIndex(ids, x)
    for k in KS:
        got, prof, st = _analogy_call(idx, call, k, method)
        assert st["filter_passes"] == 3 and st["redone_passes"] == 1, (k, st)
        assert k * 38 <= st["candidates"] <= ri.CAP * 38, (k, st)        # passes 0 and 2: 32 + 6 analogies, each k .. 8192 candidates
        assert AN_FILTER | AN_SCAN <= set(prof), (k, sorted(prof))
        assert prof["analogy_filter"] == 3 and prof["analogy_scan"] == 1 and prof["analogy_merge"] == 1, (k, prof)
        for p, t in HOT_IN_PASS_1.items():
            assert got[0][call["live"][p]].tolist() == ri.lowest_copy_ids(t, k).tolist(), (k, p)
    healthy = ri.analogy_call({}, unknown_at=())
    for k in KS:
        got, prof, st = _analogy_call(idx, healthy, k, method)
        assert st["filter_passes"] == 3 and st["redone_passes"] == 0 and k * 70 <= st["candidates"] <= ri.CAP * 70, (k, st)
        assert AN_FILTER <= set(prof) and not (AN_SCAN & set(prof)), (k, sorted(prof))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("method", METHODS)
def test_analogy_every_pass_and_the_short_last_pass_redone(gpu, method):
    x, ids = ri.table()
    idx = gpu.VectorIndex(ids, x)
    every = ri.analogy_call({5: ri.HOT_TRIPLES[0], 40: ri.HOT_TRIPLES[1], 66: ri.HOT_TRIPLES[2]})
    got, prof, st = _analogy_call(idx, every, 5, method)
    assert st == {"filter_passes": 3, "candidates": 0, "redone_passes": 3}, st
    assert prof["analogy_filter"] == 3 and prof["analogy_scan"] == 3, prof
    last = ri.analogy_call({69: ri.HOT_TRIPLES[1]})                      # the last of 70: a pass of 6, the end of the device lists
    got, prof, st = _analogy_call(idx, last, 5, method)
    assert st["filter_passes"] == 3 and st["redone_passes"] == 1 and 5 * 64 <= st["candidates"] <= ri.CAP * 64, st
    assert prof["analogy_filter"] == 3 and prof["analogy_scan"] == 1, prof
    assert got[0][last["live"][69]].tolist() == ri.lowest_copy_ids(ri.HOT_TRIPLES[1], 5).tolist()
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("method", METHODS)
def test_analogy_refining_every_row_removes_the_overflow(gpu, method):
    """check_brackets bit 3: the candidate buffer holds the whole table, so the hot pass is the filter's own work -- the same lists."""
    x, ids = ri.table()
    call = ri.analogy_call(HOT_IN_PASS_1)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("check_brackets", 8)
    before = idx.bound_checked()
    got, prof, st = _analogy_call(idx, call, 5, method)
    assert st == {"filter_passes": 3, "candidates": ri.N * 70, "redone_passes": 0}, st
    assert not (AN_SCAN & set(prof)), sorted(prof)
    assert idx.bound_checked() - before == ri.N * 70
    assert idx.bound_violations() == 0
    idx.close()


# ---- d. exact kNN: one overflowing or bad query among healthy ones ----------------------------------------------------------
@pytest.mark.parametrize("Q,at", [(70, 3), (70, 40), (70, 66), (1, 0)])
def test_search_with_one_hot_or_bad_query(gpu, oracle, knn, Q, at):
    """The query at `at` (first pass tile 0 / tile 1, the second pass of 6, a call of one) overflows its buffer, or is not finite:
    the filter ran, then the all-exact kernels answered the call; every list equals the oracle's."""
    x, ids = ri.table()
    idx = gpu.VectorIndex(ids, x)
    for bad in (None, "nan", "inf", "big"):
        qs = ri.queries(Q, hot_at=(at,), bad=bad)
        exp = _knn_expected(knn, oracle, qs, (at,), bad)
        for k in KS:
            (gi, gs), prof = _profiled(idx, lambda: idx.search(qs, k))
            assert FILTER | SCAN <= set(prof), (bad, k, sorted(prof))
            _same_lists(gi, gs, exp, k, (bad, k))
    idx.set_option("check_brackets", 4)                                  # bit 2: a buffer of N rows, every row refined -- no overflow
    qs = ri.queries(Q, hot_at=(at,))
    exp = _knn_expected(knn, oracle, qs, (at,), None)
    for k in KS:
        (gi, gs), prof = _profiled(idx, lambda: idx.search(qs, k))
        assert FILTER <= set(prof) and not (SCAN & set(prof)), (k, sorted(prof))
        _same_lists(gi, gs, exp, k, ("every row refined", k))
    assert idx.bound_violations() == 0
    idx.close()


# ---- e. what a fallback leaves behind ---------------------------------------------------------------------------------------
def test_calls_after_a_fallback_on_one_handle(gpu, oracle, knn):
    """Exact kNN and the join share two verdict words, an arrival counter and an overflow flag that a call's last workgroup leaves
    at zero.  A stale word sends every later call to the all-exact kernels (seen in the profile), or lets a call trust lists it
    must not (seen in the lists)."""
    x, ids = ri.table()
    idx = gpu.VectorIndex(ids, x)
    k = 5

    def search(qs, exp, fell_back, what):
        (gi, gs), prof = _profiled(idx, lambda: idx.search(qs, k))
        assert FILTER <= set(prof) and (SCAN <= set(prof) if fell_back else not (SCAN & set(prof))), (what, sorted(prof))
        _same_lists(gi, gs, exp, k, what)

    hot = ri.queries(hot_at=(3,))
    search(hot, _knn_expected(knn, oracle, hot, (3,), None), True, "1: a hot search")
    search(ri.queries(), knn["healthy"], False, "2: a healthy search of 70")
    nan = ri.queries(hot_at=(40,), bad="nan")
    search(nan, _knn_expected(knn, oracle, nan, (40,), "nan"), True, "3: a search with a NaN query")
    targets = ri.healthy_targets()
    (gi, gs), prof = _profiled(idx, lambda: idx.join(ri.queries(), k, targets))
    assert set(prof) == JOIN_KERNELS, ("4: a healthy join", sorted(prof))
    st = idx.last_join_stats()
    assert st["filter_queries"] == 70 and st["redone_queries"] == 0 and 70 * k <= st["candidates"] <= 70 * ri.CAP, st
    _same_lists(gi, gs, [oracle.exact_knn(x, ids, q, k, targets) for q in ri.queries()], k, "4: a healthy join")
    inf = ri.queries(hot_at=(66,), bad="inf")
    (gi, gs), prof = _profiled(idx, lambda: idx.join(inf, k, targets))
    assert SCAN <= set(prof) and idx.last_join_stats()["filter_queries"] == 0, ("5: a join with an Inf query", sorted(prof))
    _same_lists(gi, gs, [oracle.exact_knn(x, ids, q, k, targets) for q in inf], k, "5: a join with an Inf query")
    healthy = ri.analogy_call({}, unknown_at=())
    got, prof, st = _analogy_call(idx, healthy, k, "3cosadd")
    assert st["filter_passes"] == 3 and st["redone_passes"] == 0 and not (AN_SCAN & set(prof)), ("6: healthy analogies", st, sorted(prof))
    search(ri.queries(1), knn["healthy"][:1], False, "7: a healthy search of one")
    assert idx.bound_violations() == 0
    idx.close()


# ---- f. the join: overflowing queries across tiles ---------------------------------------------------------------------------
def test_join_overflow_across_tiles(gpu, oracle):
    """200 queries over 12 000 targets that hold every copy, the hot query at 6, at 127 and 128 (either side of the boundary of
    the 128-query tiles) and at 199 (the end of the second tile's tail): those four and no other are answered again.  The healthy
    ones keep the copies 0.05 below their 32nd best similarity over these targets (test_redo_inputs_cpu.py)."""
    x, ids = ri.table()
    targets = ri.overflow_targets()
    qs = ri.join_queries()
    exp = [oracle.exact_knn(x, ids, q, ri.K_MAX, targets) for q in qs]
    idx = gpu.VectorIndex(ids, x)
    for tile, k in ((0, 5), (0, 32), (64, 5)):                          # (64: tiles of 64 queries, the hot ones at their ends too)
        idx.set_option("exact_join_tile", tile)
        (gi, gs), prof = _profiled(idx, lambda: idx.join(qs, k, targets))
        st = idx.last_join_stats()
        print(f"tile option {tile}, k = {k}: {st}")
        assert JOIN_KERNELS | SCAN <= set(prof), (tile, k, sorted(prof))
        assert st["filter_queries"] == ri.JOIN_Q and st["redone_queries"] == len(ri.JOIN_HOT_AT), (tile, k, st)
        assert 196 * k <= st["candidates"] <= 196 * ri.CAP, (tile, k, st)
        _same_lists(gi, gs, exp, k, (tile, k))
        si, ss = idx.search(qs, k, subset_ids=targets)
        assert np.array_equal(gi, si) and np.array_equal(gs.view(np.uint32), ss.view(np.uint32)), (tile, k)
    assert idx.bound_violations() == 0
    idx.close()
