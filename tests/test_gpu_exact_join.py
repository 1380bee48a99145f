"""-m gpu: the exact kNN-join (exact_join.h, freddy_gpu_exact_join; the host mirror's knn_search_in_batch, grouping_func,
groups()).  Expected lists come from the oracle's exact_knn over the target set; every case is also compared bit for bit with
VectorIndex.search(..., subset_ids=targets), the call the join's contract is written against.  The handle's profile names the
kernels that ran, so a case that silently takes the other path fails."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

E_KIND = "freddy_gpu error -4"
JOIN_KERNELS = {"exact_join_gather", "exact_join_prep", "exact_join_sample", "exact_join_threshold", "exact_join_filter", "exact_join_refine"}


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


def _table(d, N, scale=1.0):
    """Clustered rows with exact duplicate rows (the generator style of test_gpu_shapes._exact_table), 200 queries."""
    x = (util.shape_corpus(N, d).numpy() * np.float32(scale)).astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]              # duplicate rows: equal similarities, ties by id
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::max(N // 200, 1)][:200].copy()
    qs[3] = -qs[3]                                  # negative similarities
    qs[6] = x[100]                                  # a query with exact copies in the table
    return x, ids, qs


def _targets(ids, N, n_known, seed=2):
    """n_known distinct known ids that hold both copies of twenty duplicated rows, 60 of them twice, 40 unknown ids; shuffled."""
    rng = np.random.default_rng(seed)
    both = np.concatenate([np.arange(100, 120), np.arange(N // 2, N // 2 + 20)])
    rest = np.setdiff1d(np.arange(N), both)
    rows = np.concatenate([both, rng.choice(rest, n_known - both.size, replace=False)])
    t = np.concatenate([ids[rows], ids[rows[:60]], np.array([4, 10**8, -7], np.int32), (ids[:37] - 1).astype(np.int32)])
    return rng.permutation(t).astype(np.int32), n_known


def _expect(oracle, x, ids, qs, kmax, targets):
    return [oracle.exact_knn(x, ids, q, kmax, targets) for q in qs]


def _same(gi, gs, exp, k, what):
    for qi, e in enumerate(exp[:gi.shape[0]]):
        e = e[:k]
        n = len(e)
        assert gi[qi, :n].tolist() == e["id"].tolist(), (what, qi)
        assert np.array_equal(gs[qi, :n].view(np.uint32), e["dist"].view(np.uint32)), (what, qi)
        assert (gi[qi, n:] == -1).all() and np.isneginf(gs[qi, n:]).all(), (what, qi)


def _same_as_search(idx, qs, k, targets, gi, gs, what):
    si, ss = idx.search(qs, k, subset_ids=targets if len(targets) else np.array([-1], np.int32))
    assert np.array_equal(gi, si) and np.array_equal(gs.view(np.uint32), ss.view(np.uint32)), what


def test_main_case(gpu, oracle):
    """20 000 x 300, 9 000 targets (8 900 distinct known rows: above the eligibility threshold), Q with tile tails, k up to the
    filter's limit, the three values of exact_filter.  No query may overflow its candidate buffer on these inputs."""
    N, d = 20000, 300
    x, ids, qs = _table(d, N)
    targets, n_known = _targets(ids, N, 8900)
    assert targets.size == 9000
    exp = _expect(oracle, x, ids, qs, 32, targets)
    idx = gpu.VectorIndex(ids, x)
    for Q in (1, 64, 70, 200):
        for k in (1, 5, 32):
            for mode in (-1, 0, 1):
                idx.set_option("exact_filter", mode)
                what = f"Q={Q} k={k} exact_filter={mode}"
                (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:Q], k, targets))
                st = idx.last_join_stats()
                _same(gi, gs, exp, k, what)
                if mode == 0:
                    assert names == {"exact_scan", "exact_merge"}, (what, sorted(names))
                    assert st == {"filter_queries": 0, "candidates": 0, "redone_queries": 0}, (what, st)
                else:
                    assert names == JOIN_KERNELS, (what, sorted(names))
                    assert st["redone_queries"] == 0 and st["filter_queries"] == Q and Q * k <= st["candidates"] <= Q * 8192, (what, st)
                _same_as_search(idx, qs[:Q], k, targets, gi, gs, what)
    idx.set_option("exact_join_tile", 64)            # the 64-query tile for a call the default answers with 128-query tiles
    idx.set_option("exact_filter", 1)
    gi, gs = idx.join(qs, 5, targets)
    _same(gi, gs, exp, 5, "tiles of 64")
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_bracket_holds_for_every_target_and_query(gpu, oracle, scale):
    """check_brackets bit 2: every (target row, query) pair is refined and its similarity compared with the MFMA value's bracket."""
    N, d = 20000, 300
    x, ids, qs = _table(d, N, scale)
    targets, n_known = _targets(ids, N, 8900)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("check_brackets", 4)
    for Q in (70, 200):
        before = idx.bound_checked()
        (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:Q], 5, targets))
        assert "exact_join_filter" in names, sorted(names)
        assert idx.bound_violations() == 0
        assert idx.bound_checked() - before == Q * n_known
        assert idx.last_join_stats() == {"filter_queries": Q, "candidates": Q * n_known, "redone_queries": 0}
        _same(gi, gs, _expect(oracle, x, ids, qs[:Q], 5, targets), 5, f"every pair, scale={scale} Q={Q}")
    idx.close()


def test_fallbacks_equal_the_oracle(gpu, oracle):
    N, d = 20000, 300
    x, ids, qs = _table(d, N)
    targets, _ = _targets(ids, N, 8900)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_filter", 1)
    for k, Q in ((33, 9), (1025, 3)):                                       # k above the filter's 32
        (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:Q], k, targets))
        assert names == {"exact_scan", "exact_merge"}, (k, sorted(names))
        _same(gi, gs, _expect(oracle, x, ids, qs[:Q], k, targets), k, f"k={k}")
        _same_as_search(idx, qs[:Q], k, targets, gi, gs, f"k={k}")
    bad = qs[:70].copy()                                                   # a query containing inf: the whole call all-exact
    bad[5, 17] = np.inf
    (gi, gs), names = _profiled(idx, lambda: idx.join(bad, 5, targets))
    assert {"exact_scan", "exact_merge"} <= names, sorted(names)
    assert idx.last_join_stats()["filter_queries"] == 0
    _same_as_search(idx, bad, 5, targets, gi, gs, "inf query")
    _same(gi, gs, _expect(oracle, x, ids, bad, 5, targets), 5, "inf query")
    idx.set_option("exact_filter", -1)                                     # below the eligibility threshold, unforced
    small = targets[:500]
    (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:70], 5, small))
    assert names == {"exact_scan", "exact_merge"}, sorted(names)
    _same(gi, gs, _expect(oracle, x, ids, qs[:70], 5, small), 5, "500 targets, unforced")
    idx.close()


def test_more_queries_than_one_pass(gpu, oracle):
    """The per-query buffers of one pass are bounded (2 GiB; here 8 896 sample floats + 8 192 candidates of 8 bytes per query:
    floor(2^31 / 101 120) rounded down to whole 128-query tiles = 21 120 queries); a call
    with more queries gathers the targets once and runs the other five launches once per pass.  Every list equals the subset
    search's; the queries either side of the pass boundary are also checked against the oracle."""
    N, d, Q = 20000, 300, 21120 + 70
    x, ids, _ = _table(d, N)
    targets, _ = _targets(ids, N, 8900)
    qs = x[(np.arange(Q) * 7) % N].copy()
    idx = gpu.VectorIndex(ids, x)
    idx.profile_enable(True)
    gi, gs = idx.join(qs, 5, targets)
    prof = idx.profile_read()
    idx.profile_enable(False)
    assert prof["exact_join_gather"][0] == 1 and prof["exact_join_filter"][0] == 2 and prof["exact_join_refine"][0] == 2, prof
    st = idx.last_join_stats()
    assert st["filter_queries"] == Q and st["redone_queries"] == 0, st
    _same_as_search(idx, qs, 5, targets, gi, gs, "two passes")
    lo = 21120 - 20
    _same(gi[lo:lo + 60], gs[lo:lo + 60], _expect(oracle, x, ids, qs[lo:lo + 60], 5, targets), 5, "around the pass boundary")
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("d", [30, 12, 516])
def test_other_d_takes_the_all_exact_path(gpu, oracle, d):
    N = 9000
    x, ids, qs = _table(d, N)
    targets, _ = _targets(ids, N, 8500)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_filter", 1)
    (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:70], 5, targets))
    assert names == {"exact_scan", "exact_merge"}, (d, sorted(names))
    _same(gi, gs, _expect(oracle, x, ids, qs[:70], 5, targets), 5, f"d={d}")
    _same_as_search(idx, qs[:70], 5, targets, gi, gs, f"d={d}")
    idx.close()


def test_edges(gpu, oracle):
    N, d = 9000, 300
    x, ids, qs = _table(d, N)
    idx = gpu.VectorIndex(ids, x)
    for mode in (-1, 1):
        idx.set_option("exact_filter", mode)
        gi, gs = idx.join(qs[:9], 4, np.empty(0, np.int32))                # the empty target set
        assert (gi == -1).all() and np.isneginf(gs).all()
        gi, gs = idx.join(qs[:9], 4, np.array([4, 10**8, -7], np.int32))   # all targets unknown
        assert (gi == -1).all() and np.isneginf(gs).all()
        few = np.array([ids[5], ids[5], ids[77], 10**8, ids[4000]], np.int32)
        gi, gs = idx.join(qs[:70], 8, few)                                 # n_targets < k
        assert (gi[:, 3:] == -1).all() and np.isneginf(gs[:, 3:]).all()
        _same(gi, gs, _expect(oracle, x, ids, qs[:70], 8, few), 8, f"three rows, k = 8, exact_filter={mode}")
        _same_as_search(idx, qs[:70], 8, few, gi, gs, "three rows")
        gi, gs = idx.join(np.empty((0, d), np.float32), 5, few)            # Q = 0
        assert gi.shape == (0, 5) and gs.shape == (0, 5)
    idx.set_option("exact_filter", 1)
    for n in (20, 31, 32, 33, 100):                                        # fewer rows than a strip / than the sample, forced filter
        t = ids[np.random.default_rng(n).choice(N, n, replace=False)]
        for k in (1, 5, 32):
            (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:70], k, t))
            assert "exact_join_filter" in names and "exact_join_refine" in names, (n, k, sorted(names))
            assert ("exact_join_sample" in names) == (n >= 32), (n, sorted(names))
            assert idx.last_join_stats()["redone_queries"] == 0
            _same(gi, gs, _expect(oracle, x, ids, qs[:70], k, t), k, f"{n} targets, k={k}, forced filter")
    pq = util.pq_tables(N=20000, K=256)
    other = gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"])
    with pytest.raises(gpu.FreddyGpuError, match=E_KIND + ".*wrong kind"):
        gpu._check(other.lib.freddy_gpu_exact_join(other.h, gpu._p(qs), 1, 1, gpu._p(ids), 1, gpu._p(np.empty(1, np.int32)), gpu._p(np.empty(1, np.float32))))
    other.close()
    assert idx.bound_violations() == 0
    idx.close()


def test_candidate_overflow_is_redone_all_exact(gpu, oracle):
    """One vector repeated 10 000 times in the target set: for the query equal to it every copy is a candidate, more than the
    8 192 a candidate buffer holds.  That query (and no list entry) is answered again by the all-exact path: ties by id."""
    N, d = 20000, 300
    x, ids, qs = _table(d, N)
    x[5000:15000] = x[4999]
    targets = np.concatenate([ids[4000:16000], np.array([4, -7], np.int32)])
    qs = qs[:70].copy()
    qs[11] = x[4999]
    idx = gpu.VectorIndex(ids, x)
    (gi, gs), names = _profiled(idx, lambda: idx.join(qs, 5, targets))
    st = idx.last_join_stats()
    assert JOIN_KERNELS <= names and "exact_scan" in names, sorted(names)
    assert st["filter_queries"] == 70 and 1 <= st["redone_queries"] < 70, st
    _same(gi, gs, _expect(oracle, x, ids, qs, 5, targets), 5, "overflow")
    _same_as_search(idx, qs, 5, targets, gi, gs, "overflow")
    assert idx.bound_violations() == 0
    idx.close()


def test_after_append_rows(gpu, oracle):
    """Targets drawn from old and appended rows: the answer of a fresh pin of the grown table.  The second append brings a larger
    element, which changes the table's operand scale the gather kernel uses."""
    d, N0, N1, N2 = 300, 12000 + 8, 12000 + 8 + 45, 12000 + 8 + 45 + 900
    x, ids, qs = _table(d, N2)
    x[N1 + 5] *= np.float32(300.0)
    idx = gpu.VectorIndex(ids[:N0], x[:N0])
    qs = np.concatenate([qs[:60], x[N0 + 3:N0 + 5], x[N1 + 5:N1 + 6]])
    rng = np.random.default_rng(4)
    for lo, n in ((N0, N1), (N1, N2)):
        idx.append_rows(ids[lo:n], vectors=x[lo:n])
        t = np.concatenate([ids[rng.choice(N0, 8600, replace=False)], ids[N0:n]])
        (gi, gs), names = _profiled(idx, lambda: idx.join(qs, 5, t))
        assert "exact_join_filter" in names, sorted(names)
        assert idx.last_join_stats()["redone_queries"] == 0
        _same(gi, gs, _expect(oracle, x[:n], ids[:n], qs, 5, t), 5, f"after the append to {n} rows")
        fresh = gpu.VectorIndex(ids[:n], x[:n])
        fi, fs = fresh.join(qs, 5, t)
        fresh.close()
        assert np.array_equal(gi, fi) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
    assert idx.bound_violations() == 0
    idx.close()


# ---- the host mirror ----------------------------------------------------------------------------------------------------------
N_DB = 20000


@pytest.fixture(scope="module")
def db():
    from freddy_amd import udf
    x = util.corpus(N_DB).numpy()
    ids_all = np.arange(1, N_DB + 1, dtype=np.int32)
    s = udf.Session()
    perm = np.random.default_rng(1).permutation(N_DB)
    s.load_vecs_norm(ids_all[perm], x[perm])
    pq = util.pq_tables(N=N_DB, K=256)
    s.load_pq(pq["codebook"], pq["ids"][perm], pq["codes"][perm])
    yield s, x
    s.close()


def _rows3_equal(rows, exp):
    assert rows["query_id"].tolist() == [r[0] for r in exp]
    assert rows["id"].tolist() == [r[1] for r in exp]
    assert np.array_equal(rows["distance"].view(np.uint32), np.array([r[2] for r in exp], np.float32).view(np.uint32))


def test_knn_search_in_batch_is_knn_in_exact_per_query(db):
    s, x = db
    rng = np.random.default_rng(5)
    targets = np.concatenate([rng.choice(np.arange(1, N_DB + 1), 9000, replace=False), [17, 17, N_DB + 5, -3]]).astype(np.int32)
    qids = np.array([11, 500, 7777, 42, 19999], np.int32)
    qs = x[qids - 1]
    for t, k in ((targets, 5), (targets[:300], 5), (np.array([9, 9, 12, N_DB + 1], np.int32), 4)):
        exp = []
        for i, q in enumerate(qs):
            exp += [(i + 1, int(r["id"]), r["distance"]) for r in s.knn_in_exact(q, k, t)]
        _rows3_equal(s.knn_search_in_batch(qs, k, t), exp)
    # the varchar[] form: an unknown query id has no rows, a repeated one is answered each time, in argument order
    by_id = np.array([500, N_DB + 9, 11, 500], np.int32)
    exp = []
    for qid in by_id:
        if 1 <= qid <= N_DB:
            exp += [(int(qid), int(r["id"]), r["distance"]) for r in s.knn_in_exact(x[qid - 1], 5, targets)]
    _rows3_equal(s.knn_search_in_batch_ids(by_id, 5, targets), exp)
    assert len(s.knn_search_in_batch_ids([N_DB + 9], 5, targets)) == 0


def test_grouping_func_and_groups(db):
    s, x = db
    rng = np.random.default_rng(6)
    tokens = np.concatenate([rng.choice(np.arange(1, N_DB + 1), 150, replace=False), [N_DB + 2, 33, 33]]).astype(np.int32)
    groups = np.array([5, 900, 12345, 19000, 901, N_DB + 7], np.int32)
    exp = []
    for tok in np.unique(tokens):
        if tok <= N_DB:
            r = s.knn_in_exact(x[tok - 1], 1, groups)
            exp.append((int(tok), int(r["id"][0])))
    got = s.grouping_func(tokens, groups)
    assert list(zip(got["id"].tolist(), got["group_id"].tolist())) == exp
    assert s.get_groups_function_name() == "grouping_func"
    assert np.array_equal(s.groups(tokens, groups), got)
    assert len(s.grouping_func(tokens, [N_DB + 7])) == 0          # no group is a row: knn_in is empty, the join has no rows
    s.set_groups_function("grouping_func_pq")
    known = groups[:-1]
    assert np.array_equal(s.groups(tokens, known), s.grouping_pq(tokens, known))
    s.set_groups_function("grouping_func")


def test_cluster_exact_did_not_move(db, oracle):
    """cluster_exact with a fixed draws sequence against the Python restatement of generic_cluster the existing cluster test
    uses (rows from the oracle's exact_knn), now that its kNN rows come from freddy_gpu_exact_join."""
    from test_gpu_udf import _cluster_reference
    s, x = db
    rng = np.random.default_rng(32)
    tokens = np.sort(rng.choice(np.arange(1, N_DB + 1), 120, replace=False)).astype(np.int32)
    vecs, k, n = x[tokens - 1], 6, 120
    draws = rng.random(k + 9 * k * 10)

    def rows_exact(cent):
        out = []
        for qi, c in enumerate(cent):
            e = oracle.exact_knn(x, np.arange(1, N_DB + 1, dtype=np.int32), c, n, tokens)
            out += [(np.float32(e["dist"][r]), qi + 1, int(np.searchsorted(tokens, e["id"][r])) + 1) for r in range(len(e))]
        return out

    exp = _cluster_reference(rows_exact, vecs, n, k, draws)
    got = s.cluster_exact(tokens, k, draws)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
