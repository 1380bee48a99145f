"""CPU check of tests/width_inputs.py: the conditions under which tests/test_gpu_selection_widths.py means something.  The case
lists reach every selection width of every dispatch family at both sides of every rung (computed from the lists: deleting a
case fails here); the tie groups hold more equal keys than a list keeps, the tables hold more candidates than a list is long,
the far query and the small sentinels do what they are there for -- all of it said by the oracle, nothing here needs a device."""
import os
import re

import numpy as np
import pytest

import width_inputs as wi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "postgres-word2vec_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the ladder and the case lists ------------------------------------------------------------------------------------------
def test_ladder_is_the_sources():
    """pick_V of csrc/generic.hip, read from the source: the restatement in width_inputs.py has the same rungs."""
    src = open(os.path.join(CSRC, "generic.hip")).read()
    body = src[src.index("int pick_V(int L) {"):]
    body = body[:body.index("\n}")]
    rungs = [(int(a), int(b)) for a, b in re.findall(r"if \(L <= (\d+)\) return (\d+);", body)]
    assert rungs == list(zip(wi.RUNGS, wi.WIDTHS)), rungs
    assert [wi.pick_V(L) for L in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 0]


@pytest.mark.parametrize("family", sorted(wi.FAMILIES))
def test_case_list_reaches_every_width_and_both_sides_of_every_rung(family):
    assert wi.coverage_gaps(family) == []


@pytest.mark.parametrize("family", sorted(wi.FAMILIES))
def test_deleting_any_case_leaves_a_gap(family):
    """Every listed case is the only one at its side of its rung: without it coverage_gaps() names what is missing."""
    cases = wi.FAMILIES[family][0]
    for c in cases:
        assert wi.coverage_gaps(family, [o for o in cases if o != c]), (family, c)


def test_exact_join_has_one_k_per_width():
    assert [wi.pick_V(k) for k in wi.EXACT_JOIN_K] == list(wi.WIDTHS)
    assert all(k == 64 * wi.pick_V(k) for k in wi.EXACT_JOIN_K)


# ---- A. IVFADC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(wi.SHAPES))
def test_ivfadc_tie_group_rows_and_rounds(oracle, key):
    t = wi.ivf_table(key)
    qs = wi.ivf_queries(key)
    ot = oracle.ivf_table(*wi.ivf_pin_args(t))
    sizes = np.diff(t["list_off"])
    assert sorted(sizes.tolist(), reverse=True) == list(wi.IVF_SIZES) and t["ids"].size == 6000
    pos = t["tie_pos"]
    big = int(np.argmax(sizes))
    assert pos.size == 2 * max(wi.TIE_K) + 3 and (t["codes"][pos] == t["codes"][pos[0]]).all()
    assert t["list_off"][big] <= pos[0] and pos[-1] < t["list_off"][big + 1]
    between = t["ids"][pos[:-1] + 1]
    assert (t["ids"][pos[:-1]] < between).all() and (between < t["ids"][pos[1:]]).all(), "the group's ids are not interleaved"
    tie = qs[wi.TIE_AT][None, :]
    same = t["ids"][(t["codes"] == t["codes"][pos[0]]).all(1)]    # (K = 16, m = 8: a few other rows have the group's code row by chance)
    assert same.size < pos.size + 40
    for W in wi.IVF_W:
        for k in wi.TIE_K:
            wide = oracle.ivfadc_search_many(ot, tie, 2 * k + 2, W, sentinel=1000.0, found_rule=0)
            assert _bits(wide["dist"][:, 0]) == _bits(wide["dist"][:, 2 * k + 1]), (key, W, k)
            assert np.isin(wide["id"], same).all(), (key, W, k)
    # enough rows: with every list probed each query has more than L = 1026 rows under the sentinel of 1000; with W = 1 the tie
    # query's first list is the largest one; queries whose first list is shorter than k carry their list into further rounds
    L = 2 * max(wi.K2)
    full = oracle.ivfadc_search_many(ot, qs, L + 1, wi.IVF_C, sentinel=1000.0, found_rule=0)
    assert (full["id"] >= 0).all() and (full["dist"] < 1000.0).all()
    one, found, rounds = oracle.ivfadc_search_many(ot, qs, L + 1, 1, sentinel=1000.0, found_rule=0, max_rounds=1)
    assert (one["id"][wi.TIE_AT] >= 0).all() and sizes[big] > L
    for k in (257, 513):                                        # (lists of 150 rows, and of 350)
        _, _, rounds = oracle.ivfadc_search_many(ot, qs, k, 1, sentinel=1000.0, found_rule=0, max_rounds=0)
        assert rounds.min() == 1 and rounds.max() >= 2, (key, k, rounds)
    # the sentinel inside the data: under the accepted-rows rule lists of every k end in padding entries for some query and
    # hold rows for every query (fewer rows than k)
    rule, sent = wi.ivf_settings(key)[1]
    assert rule == 1 and 0.0 < sent < 1000.0
    for k in (min(wi.K2), max(wi.K2)):
        e = oracle.ivfadc_search_many(ot, qs, k, wi.IVF_C, sentinel=sent, found_rule=rule)
        assert (e["id"][:, 0] >= 0).sum() >= 4 and (e["id"][:, -1] < 0).any() and (e["dist"][e["id"] < 0] == np.float32(sent)).all(), (key, k)
        assert (e["id"][wi.TIE_AT] >= 0).all(), "the tie group lies under the sentinel"


# ---- B. flat PQ --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(wi.SHAPES))
def test_pq_tie_group_and_rows(oracle, key):
    t = wi.pq_table(key)
    qs = wi.pq_queries(key)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    pos = t["tie_pos"]
    assert t["ids"].size == wi.PQ_N > 2 * max(wi.K2) and pos[-1] < wi.PQ_N and (np.diff(t["ids"]) > 0).all()
    assert (t["codes"][pos] == t["codes"][pos[0]]).all() and (np.diff(pos) == 2).all()
    for k in wi.TIE_K:
        wide = oracle.pq_search(ot, qs[wi.TIE_AT], 2 * k + 2)
        assert _bits(wide["dist"][0]) == _bits(wide["dist"][2 * k + 1]) and np.isin(wide["id"], t["ids"][pos]).all(), (key, k)
    full = np.stack([oracle.pq_search(ot, q, 2 * max(wi.K2) + 1) for q in qs])
    assert (full["id"] >= 0).all() and (full["dist"] < wi.PQ_SENTINEL).all()
    sub = wi.pq_small_subset()
    known = np.unique(sub[np.isin(sub, t["ids"])])
    assert known.size == 20 < min(wi.K2) and np.isin(known, t["ids"][pos]).sum() >= 4
    e = oracle.pq_search_in(ot, qs[0], min(wi.K2), sub)
    assert (e["id"][:20] >= 0).all() and (e["id"][20:] < 0).all()


# ---- C. probe plan -------------------------------------------------------------------------------------------------------------
def test_probe_table_far_query_ties_and_rounds(oracle):
    t = wi.probe_table()
    qs = wi.probe_queries()
    ot = oracle.ivf_table(*wi.ivf_pin_args(t))
    sizes = np.diff(t["list_off"])
    assert sizes.size == wi.PROBE_C and sizes.max() <= 12 and (sizes[list(wi.PROBE_EMPTY)] == 0).all() and (sizes > 0).sum() > 480
    assert t["coarse"].shape == (wi.PROBE_C, 64) and 2 * max(wi.PROBE_W) == 1024 and max(wi.PROBE_W) < wi.PROBE_C
    for a, b in wi.PROBE_DUP:
        assert np.array_equal(_bits(t["coarse"][a]), _bits(t["coarse"][b]))
    dist = wi.probe_distances(oracle)
    near = (dist < np.float32(wi.CELL_LIMIT)).sum(1)
    assert 1 <= near[wi.PROBE_FAR] < min(wi.PROBE_W), near
    assert (np.delete(near, wi.PROBE_FAR) == wi.PROBE_C).all(), near
    # a tied pair of centroids inside the W nearest cells of a query, at the smallest and at a middle W
    order = np.argsort(dist, axis=1, kind="stable")             # (distance, cell) ascending: the order the plan replays
    rank = np.argsort(order, axis=1)
    for W in (min(wi.PROBE_W), 129):
        inside = [(q, a, b) for q in range(qs.shape[0]) for a, b in wi.PROBE_DUP if rank[q, a] < W and rank[q, b] < W]
        assert inside, W
        assert all(dist[q, a] == dist[q, b] for q, a, b in inside)
    # at every bound W of the ladder query PROBE_EDGE has two equally near cells at the W-th place: ranks W - 1 and W
    assert set(wi.PROBE_EDGE_W) == {W for W in wi.PROBE_W if 2 * W in wi.RUNGS} and all(W + 1 in wi.PROBE_W for W in wi.PROBE_EDGE_W[:-1])
    for W in wi.PROBE_EDGE_W:
        a, b = order[wi.PROBE_EDGE, W - 1], order[wi.PROBE_EDGE, W]
        assert dist[wi.PROBE_EDGE, a] == dist[wi.PROBE_EDGE, b] < wi.CELL_LIMIT and a < b, (W, a, b)
        assert np.array_equal(_bits(t["coarse"][a]), _bits(t["coarse"][b])) and 0 < sizes[a] != sizes[b] > 0, (W, a, b)   # (lists of different lengths: the choice shows in the rows read)
    # the small sentinel sends queries into further rounds: at W >= 257 the second round has fewer than W cells left
    rule, sent = wi.probe_settings()[1]
    for W in (32, 257, 512):
        _, found, rounds = oracle.ivfadc_search_many(ot, qs, wi.PROBE_K, W, sentinel=sent, found_rule=rule, max_rounds=0)
        assert rounds.max() >= 2, (W, rounds, found)
    # under the reference's rule every query ends with round one at every W (the rows that round read are then what the handle
    # reports), and the tie at the W-th place changes that number
    for W in wi.PROBE_W:
        _, found, rounds = oracle.ivfadc_search_many(ot, qs, wi.PROBE_K, W, sentinel=1000.0, found_rule=0, max_rounds=0)
        assert (rounds == 1).all() and (np.delete(found, wi.PROBE_FAR) > 2 * wi.PROBE_K).all(), (W, rounds, found)
    # fewer rows than k: the cells the far query can reach hold fewer than PROBE_FEW_K rows (its list ends in padding entries at
    # every W), every other query has that many
    reach = int(sizes[dist[wi.PROBE_FAR] < np.float32(wi.CELL_LIMIT)].sum())
    assert 0 < reach < wi.PROBE_FEW_K < t["ids"].size, reach
    for W in (min(wi.PROBE_W), max(wi.PROBE_W)):
        e = oracle.ivfadc_search_many(ot, qs, wi.PROBE_FEW_K, W, sentinel=1000.0, found_rule=0)
        assert ((e["id"] >= 0).sum(1) == np.where(np.arange(qs.shape[0]) == wi.PROBE_FAR, reach, wi.PROBE_FEW_K)).all(), W
    for W in wi.PROBE_EDGE_W:
        a, b = order[wi.PROBE_EDGE, W - 1], order[wi.PROBE_EDGE, W]
        rows = wi.probe_round_one_rows(oracle, ot, W)[wi.PROBE_EDGE]
        nearer = int(sizes[order[wi.PROBE_EDGE, :W - 1]].sum())
        assert rows - nearer in (sizes[a], sizes[b]) and sizes[a] != sizes[b], (W, rows, nearer, sizes[a], sizes[b])
        if W + 1 in wi.PROBE_W:
            assert wi.probe_round_one_rows(oracle, ot, W + 1)[wi.PROBE_EDGE] == nearer + sizes[a] + sizes[b], W


# ---- D. exact kNN ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", wi.EXACT_D)
def test_exact_copies_and_subsets(oracle, d):
    x, ids = wi.exact_table(d)
    qs = wi.exact_queries(d)
    copies = np.nonzero((x == qs[wi.EXACT_TIE]).all(1))[0]
    assert ids.size == 3051 > max(wi.EXACT_K) and copies.size >= wi.EXACT_COPIES == 2 * 1024 + 3
    gaps = np.diff(copies)
    assert (gaps > 1).sum() > 300, "the copies' ids are not interleaved with other rows'"
    wide = oracle.exact_knn(x, ids, qs[wi.EXACT_TIE], 2 * 1024 + 2)
    assert _bits(wide["dist"][0]) == _bits(wide["dist"][2 * 1024 + 1]) and wide["id"].tolist() == ids[copies[:2050]].tolist()
    # the negated query: the copies are its LAST rows, so its longest lists and its list over the small subset hold negative similarities
    assert np.array_equal(qs[wi.EXACT_NEG], -qs[wi.EXACT_TIE])
    assert oracle.exact_knn(x, ids, qs[wi.EXACT_NEG], 1024)["dist"][-1] < 0.0, "no negative similarity in the negated query's list"
    subs = wi.exact_subsets(d)
    known = {name: np.unique(s[np.isin(s, ids)]).size for name, s in subs.items()}
    assert known == {"large": 1500, "small": 50, "join": 2000}
    assert known["large"] > max(wi.EXACT_K) and known["small"] < min(wi.EXACT_K) and known["join"] > max(wi.EXACT_JOIN_K)
    assert all((~np.isin(s, ids)).any() and np.unique(s).size < s.size for s in subs.values()), "unknown ids and duplicates"
    assert len(oracle.exact_knn(x, ids, qs[0], min(wi.EXACT_K), subs["small"])) == 50
    assert oracle.exact_knn(x, ids, qs[wi.EXACT_NEG], min(wi.EXACT_K), subs["small"])["dist"][-1] < 0.0
    assert max(wi.EXACT_Q) == qs.shape[0] and 8 in wi.EXACT_Q and 9 in wi.EXACT_Q


# ---- E, F, G. the kNN-join -------------------------------------------------------------------------------------------------------
def test_join_tables_targets_and_equal_codewords(oracle):
    qs = wi.join_queries()
    targets = wi.join_targets()
    known = np.unique(targets[(targets >= 1) & (targets <= wi.JOIN_N)])
    assert known.size == 3000 > max(max(wi.FAMILIES["join_m01"][1](k) for k in wi.JOIN_K), max(k * p for k, p in wi.JOIN_PV))
    assert targets.size == 3032 and qs.shape == (wi.JOIN_Q, 64)
    few = wi.join_few_targets()
    assert few.size == 20 < min(wi.JOIN_FEW["k"], wi.SIDE_CALL["k"] * 3) and wi.SIDE_FEW in wi.SIDE_KC
    for kc in (wi.JOIN_QUERY_KC, 129):
        t = wi.ivpq_table(kc, True)
        c = t["coarse"]
        assert c.shape == (2, kc, 32) and t["coarse_id"].max() < kc * kc and t["stats"].size == kc * kc + 1
        for h, a, b in ((0, kc - 1, 1), (0, kc // 2, 0), (1, kc - 2, 0), (1, kc // 2 + 1, 2)):
            assert a != b and np.array_equal(_bits(c[h, a]), _bits(c[h, b]))
        assert abs(float(t["stats"][:-1].sum()) - 1.0) < 1e-3 and t["stats"][-1] == wi.JOIN_N
    # equal keys inside the taken prefix: for some query the cells the oracle selects hold both members of a copied pair of the
    # first half (cells c0 = 1 and c0 = kc - 1 beside the same c1)
    kc = wi.JOIN_QUERY_KC
    ot = oracle.ivpq_table(*wi.ivpq_pin_args(wi.ivpq_table(kc, True)))
    sel, _ = oracle.multi_index_select(ot, qs, np.arange(wi.JOIN_Q), targets.size, 512 * wi.JOIN_ALPHA, wi.JOIN_CONF)
    both = [q for q, cells in enumerate(sel)
            if any(c % kc == 1 and (c - 1 + kc - 1) in set(cells.tolist()) for c in cells.tolist())]
    assert both, [len(s) for s in sel]
    # full selections: in round one of every query-kernel case the target rows of the cells a query takes outnumber the L keys
    # its selection keeps, for most queries (method 2: alpha = 2 pvf; methods 0 / 1: 3k expected targets against 2k keys)
    tbl = wi.ivpq_table(kc, True)
    per_cell = np.bincount(tbl["coarse_id"][known - 1], minlength=kc * kc)
    for L, min_target in [(2 * k, k * wi.JOIN_ALPHA) for k in wi.JOIN_K] + [(k * p, k * wi.join_pv_alpha(p)) for k, p in wi.JOIN_PV]:
        assert min_target < known.size
        sel, _ = oracle.multi_index_select(ot, qs, np.arange(wi.JOIN_Q), targets.size, min_target, wi.JOIN_CONF)
        cand = np.array([per_cell[cells].sum() for cells in sel])
        assert (cand > L).sum() >= wi.JOIN_Q // 2, (L, min_target, cand.tolist())


@pytest.mark.parametrize("kc", wi.TRAVERSE_KC)
def test_traversal_tables_and_deep_stops(oracle, kc):
    """The traversal tables have distinct codewords in both halves (equal ones would hand queries back to the host heap).  The
    deep call's first-round stop lies beyond 63 cells for a query none of whose cells are equally far -- the device answers it
    itself, with the sort over all 64 V keys and the chunks behind the first -- and within 64 cells for the other two calls."""
    t = wi.ivpq_table(kc, False)
    for h in range(2):
        assert len({r.tobytes() for r in t["coarse"][h]}) == kc, (kc, h)
    ot = oracle.ivpq_table(*wi.ivpq_pin_args(t))
    qs, n_targets = wi.join_queries(), wi.join_targets().size
    free = wi.tie_free_queries(oracle, kc)
    near, within, deep = wi.traverse_calls(kc)
    assert deep == wi.TRAVERSE_DEEP and not wi.traverse_small(*deep, n_targets, kc * kc)
    for k, alpha in (near, within):
        sel, _ = oracle.multi_index_select(ot, qs, np.arange(wi.JOIN_Q), n_targets, k * alpha, wi.JOIN_CONF)
        assert max(len(s) for s in sel) <= 63, (kc, k, alpha)
    sel, _ = oracle.multi_index_select(ot, qs, np.arange(wi.JOIN_Q), n_targets, deep[0] * deep[1], wi.JOIN_CONF)
    taken = np.array([len(s) for s in sel])
    for q in free:                                               # (the oracle's order of taken cells is the ascending key order)
        keys = wi.cell_keys(oracle, t, qs[q])
        assert sel[q].tolist() == np.lexsort((np.arange(kc * kc), keys))[:taken[q]].tolist(), (kc, q)
    if wi.pick_V(kc * kc) > 1:
        assert (taken[free] > 63).any() and (taken < kc * kc).all(), (kc, taken.tolist(), free)


def test_traversal_calls_take_both_kernels_at_every_width():
    """For every traversal width above 1 the case list holds a call with `small` true and one with it false (join_run.h
    launch_traverse, restated in width_inputs.traverse_small); a width of 1 has no SMALL kernel."""
    n = wi.join_targets().size
    seen = {}
    for kc in wi.TRAVERSE_KC:
        calls = wi.traverse_calls(kc)
        flags = [wi.traverse_small(k, alpha, n, kc * kc) for k, alpha in calls]
        tv = wi.pick_V(kc * kc)
        assert flags == ([False, False, False] if tv == 1 else [True, False, False]), (kc, calls, flags)
        assert all(k * alpha < 3000 for k, alpha in calls), (kc, calls)       # (min_target stays below the known targets)
        seen.setdefault(tv, set()).update(flags)
    assert seen == {1: {False}, 2: {True, False}, 4: {True, False}, 8: {True, False}, 16: {True, False}}
