"""-m gpu: every WaveSelect<V> instantiation of every dispatch family, at both sides of every rung of the ladder (pick_V:
L <= 64 -> 1, 128 -> 2, 256 -> 4, 512 -> 8, 1024 -> 16).  Inputs and case lists come from tests/width_inputs.py;
tests/test_width_inputs_cpu.py proves that the lists reach every (family, V, side of rung) and that the tie groups, row counts,
far query and sentinels are what the cases need.  Every comparison is bit for bit against the CPU oracle given the same arrays
(ids, ranks, float bits); where a handle keeps a profile it names the kernels that ran, so a case that silently takes another
family's kernels fails.  (The kNN-join launches without the profile: its widths are a function of the arguments alone.)"""
import contextlib

import numpy as np
import pytest

import util
import width_inputs as wi

pytestmark = pytest.mark.gpu

E_LIMIT = "freddy_gpu error -5"   # include/freddy_gpu.h FREDDY_E_LIMIT as gpu._check words it


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def pins(gpu, oracle):
    """(handle, oracle table) per table of width_inputs, pinned once per module."""
    made = {}

    def get(kind, key):
        if (kind, key) not in made:
            if kind == "ivf":
                t = wi.ivf_table(key) if key != "probe" else wi.probe_table()
                made[kind, key] = (gpu.IVFIndex(*wi.ivf_pin_args(t)), oracle.ivf_table(*wi.ivf_pin_args(t)))
            elif kind == "pq":
                t = wi.pq_table(key)
                made[kind, key] = (gpu.PQIndex(t["codebook"], t["ids"], t["codes"]), oracle.pq_table(t["codebook"], t["ids"], t["codes"]))
            elif kind == "vec":
                x, ids = wi.exact_table(key)
                made[kind, key] = (gpu.VectorIndex(ids, x), None)
            else:
                t = wi.ivpq_table(*key)
                made[kind, key] = (gpu.IVPQIndex(*wi.ivpq_pin_args(t)), oracle.ivpq_table(*wi.ivpq_pin_args(t)))
        return made[kind, key]

    yield get
    for idx, _ in made.values():
        idx.close()


@contextlib.contextmanager
def _option(idx, name, value, default=-1):
    """An option of a handle for the length of a block; the default comes back whether or not the block's assertions hold (the
    handles are shared by the parametrised cases)."""
    idx.set_option(name, value)
    try:
        yield
    finally:
        idx.set_option(name, default)


@contextlib.contextmanager
def _pinned_ivpq(gpu, oracle, t):
    """(handle, oracle table) of a table that one case pins for itself; unpinned when the case ends, however it ends."""
    idx = gpu.IVPQIndex(*wi.ivpq_pin_args(t))
    try:
        yield idx, oracle.ivpq_table(*wi.ivpq_pin_args(t))
    finally:
        idx.close()


def _profiled(idx, call):
    """(result of call(), names of the kernels it launched)"""
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _scan_family(names, k, what):
    """The generic scan ran: adc_scan + merge_replay up to k = 512, the selection passes + bigk_replay from 513 on."""
    assert "adc_scan" in names and "lut_build" in names, (what, sorted(names))
    assert not names & {"ivf_filter", "ivf_multi_scan", "ivf_exact_scan", "ivf_one", "pq_front", "pq_one", "merge_refine", "merge_surv"}, (what, sorted(names))
    assert ("merge_replay" in names) == (k <= 512) and ("bigk_replay" in names) == (k > 512), (what, sorted(names))


# ---------------------------------------------------------------------------------------
# A. IVFADC, generic scan: adc_scan_kernel<12 | 0, V> + merge_replay_kernel<V>, L = 2k
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", wi.K2)
@pytest.mark.parametrize("key", sorted(wi.SHAPES))
def test_ivfadc_generic_scan(pins, oracle, key, k):
    """Every list probed (W = C) and one per round (W = 1: lists of 150 .. 2300 rows, so some queries carry their list over
    rounds); the reference's found rule with its sentinel and the accepted-rows rule with a sentinel inside the data (lists that
    end in padding entries); query 3 meets 1027 equal distances.  Through the host-buffer call."""
    idx, ot = pins("ivf", key)
    qs = wi.ivf_queries(key)
    with _option(idx, "fused", 0):                    # (k = 32 alone could take a cell-grouped scan: L = 64)
        for W in wi.IVF_W:
            for rule, sent in wi.ivf_settings(key):
                what = f"ivfadc shape={wi.SHAPES[key]} k={k} W={W} rule={rule} sentinel={sent}"
                exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
                (gi, gd), names = _profiled(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule))
                util.assert_same_lists(gi, gd, exp, what)
                _scan_family(names, k, what)
                assert "probe_plan" in names, (what, sorted(names))
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("k", wi.IVF_DEV_K)
@pytest.mark.parametrize("key", sorted(wi.SHAPES))
def test_ivfadc_generic_scan_device_pointers(pins, oracle, key, k):
    """The rung 256 | 258 keys again through freddy_gpu_ivfadc_search_dev: round one's lists, every list probed."""
    import torch
    idx, ot = pins("ivf", key)
    qs = wi.ivf_queries(key)
    dev = torch.device("cuda", 0)
    for rule, sent in wi.ivf_settings(key):
        exp, _, _ = oracle.ivfadc_search_many(ot, qs, k, wi.IVF_C, sentinel=sent, found_rule=rule, max_rounds=1)
        dq = torch.from_numpy(np.array(qs, np.float32)).to(dev)
        oi = torch.full((qs.shape[0], k), -7, dtype=torch.int32, device=dev)
        od = torch.full((qs.shape[0], k), -3.0, dtype=torch.float32, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _, names = _profiled(idx, lambda: idx.search_dev(dq.data_ptr(), qs.shape[0], k, wi.IVF_C, sent, rule, oi.data_ptr(), od.data_ptr(), st.data_ptr()))
        torch.cuda.synchronize(dev)
        what = f"ivfadc_search_dev shape={wi.SHAPES[key]} k={k} rule={rule}"
        util.assert_same_lists(oi.cpu().numpy(), od.cpu().numpy(), exp, what)
        _scan_family(names, k, what)
    assert idx.bound_violations() == 0


# ---------------------------------------------------------------------------------------
# B. flat PQ: the same kernels from pq_chunk, L = min(2k, 1024)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", wi.K2)
@pytest.mark.parametrize("key", sorted(wi.SHAPES))
def test_pq_generic_scan(pins, oracle, key, k):
    """The whole table of 3000 rows (query 3 meets 1027 equal distances) and a subset of 20 rows, fewer than k: the rest of the
    list stays padding."""
    idx, ot = pins("pq", key)
    qs = wi.pq_queries(key)
    what = f"pq shape={wi.SHAPES[key]} k={k}"
    with _option(idx, "pq_fused", 0):
        exp = np.stack([oracle.pq_search(ot, q, k) for q in qs])
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs, k, sentinel=wi.PQ_SENTINEL))
        util.assert_same_lists(gi, gd, exp, what)
        _scan_family(names, k, what)
        sub = wi.pq_small_subset()
        exp = np.stack([oracle.pq_search_in(ot, q, k, sub) for q in qs])
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs, k, sentinel=1000.0, subset_ids=sub))
        util.assert_same_lists(gi, gd, exp, what + " subset of 20 rows")
        assert (gi[:, 20:] == -1).all() and (gi[:, :20] >= 0).all(), what
        _scan_family(names, k, what)
        assert "gather_rows" in names, (what, sorted(names))


# ---------------------------------------------------------------------------------------
# C. probe plan: probe_plan_kernel<V>, L = 2W
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", wi.PROBE_W)
def test_probe_plan(pins, oracle, W):
    """520 cells of at most 12 rows, four of them empty, three centroids copies of others; 8 queries (fewer than 32: the fp32
    plan kernel, not the MFMA cell selection), one of them with fewer than 32 cells inside the cell limit.  The small sentinel
    of the second setting sends queries into further rounds: from W = 257 on the second round finds fewer than W cells left.
    Query 0 has two equally near cells at the W-th place for W = 32, 64, 128, 256, 512, with lists of different lengths: the
    rows that round one read say which of them the plan took.  The cell-grouped scan (fused = 1) and the generic one (0) behind
    the same plan."""
    idx, ot = pins("ivf", "probe")
    qs = wi.probe_queries()
    k = wi.PROBE_K
    for rule, sent in wi.probe_settings():
        exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
        for fused in (1, 0):
            what = f"probe plan W={W} rule={rule} sentinel={sent} fused={fused}"
            with _option(idx, "fused", fused):
                (gi, gd), names = _profiled(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule))
                util.assert_same_lists(gi, gd, exp, what)
                assert "probe_plan" in names and "coarse_dist" in names and "coarse_table" not in names, (what, sorted(names))
                assert ("ivf_multi_scan" in names) == (fused == 1) and ("adc_scan" in names) == (fused == 0), (what, sorted(names))
                if rule == 0:   # (every query ends with round one: the rows its cells hold are the plan's own output)
                    assert idx.last_scanned_rows() == int(wi.probe_round_one_rows(oracle, ot, W).sum()), what
    # fewer rows than k: the cells the far query can reach hold fewer than PROBE_FEW_K rows, its list ends in padding entries
    what = f"probe plan W={W} k={wi.PROBE_FEW_K}"
    exp = oracle.ivfadc_search_many(ot, qs, wi.PROBE_FEW_K, W, sentinel=1000.0, found_rule=0)
    (gi, gd), names = _profiled(idx, lambda: idx.search(qs, wi.PROBE_FEW_K, W, sentinel=1000.0, found_rule=0))
    util.assert_same_lists(gi, gd, exp, what)
    assert "probe_plan" in names and (gi[wi.PROBE_FAR, -1] < 0) and (np.delete(gi, wi.PROBE_FAR, axis=0) >= 0).all(), (what, sorted(names))
    assert idx.bound_violations() == 0


# ---------------------------------------------------------------------------------------
# D. exact kNN: exact_scan_kernel<V, QT> + exact_merge_kernel<V>, L = min(k, 1024); the exact join's all-exact path
# ---------------------------------------------------------------------------------------
_exact_expected = {}


def _exact_lists(oracle, d, sub):
    """The oracle's lists of 1025 entries for the 20 queries (ORDER BY similarity DESC, id ASC is a total order: the list for k
    is their prefix), computed once per (d, subset)."""
    if (d, sub) not in _exact_expected:
        x, ids = wi.exact_table(d)
        s = None if sub is None else wi.exact_subsets(d)[sub]
        _exact_expected[d, sub] = [oracle.exact_knn(x, ids, q, max(wi.EXACT_K), s) for q in wi.exact_queries(d)]
    return _exact_expected[d, sub]


@pytest.mark.parametrize("k", wi.EXACT_K)
@pytest.mark.parametrize("d", wi.EXACT_D)
def test_exact_knn(pins, oracle, d, k):
    """3051 rows, 2051 of them one vector; 1, 8, 9 and 20 queries (tiles of 8; of 16 from 9 queries on up to V = 4); query 6 is
    the copied vector (2051 equal similarities), query 3 its negative; the whole table, a subset of 1500 rows and one of 50
    (fewer than k: padding)."""
    idx, _ = pins("vec", d)
    qs = wi.exact_queries(d)
    for sub in (None, "large", "small"):
        exp = _exact_lists(oracle, d, sub)
        s = None if sub is None else wi.exact_subsets(d)[sub]
        for Q in wi.EXACT_Q:
            what = f"exact d={d} k={k} Q={Q} subset={sub}"
            (gi, gs), names = _profiled(idx, lambda: idx.search(qs[:Q], k, subset_ids=s))
            assert "exact_scan" in names and "exact_merge" in names and "exact_filter" not in names, (what, sorted(names))
            util.assert_exact_lists(gi, gs, exp, k, what)
            if sub == "small":
                assert (gi[:, 50:] == -1).all() and (gi[:, :50] >= 0).all(), what
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("d", wi.EXACT_D)
def test_exact_join_all_exact_path(pins, oracle, d):
    """freddy_gpu_exact_join over 2000 known targets (with duplicates and unknown ids), one k per width: k > 32 takes the
    all-exact path whatever the size of the set."""
    idx, _ = pins("vec", d)
    qs = wi.exact_queries(d)
    exp = _exact_lists(oracle, d, "join")
    targets = wi.exact_subsets(d)["join"]
    for k in wi.EXACT_JOIN_K:
        for Q in (9, 20):
            (gi, gs), names = _profiled(idx, lambda: idx.join(qs[:Q], k, targets))
            what = f"exact join d={d} k={k} Q={Q}"
            assert "exact_scan" in names and "exact_merge" in names and not {n for n in names if "filter" in n}, (what, sorted(names))
            util.assert_exact_lists(gi, gs, exp, k, what)
        (gi, gs), names = _profiled(idx, lambda: idx.join(qs, k, wi.exact_subsets(d)["small"]))      # 50 targets: fewer rows than k
        assert "exact_scan" in names and not {n for n in names if "filter" in n}, (k, sorted(names))
        util.assert_exact_lists(gi, gs, _exact_lists(oracle, d, "small"), k, f"exact join d={d} k={k} over 50 targets")
        assert (gi[:, 50:] == -1).all() and (gi[:, :50] >= 0).all(), k
    assert idx.last_join_stats()["filter_queries"] == 0
    assert idx.bound_violations() == 0


# ---------------------------------------------------------------------------------------
# E. kNN-join, query kernel: join_query_kernel<V>, L = 2k (methods 0, 1) or k pvf (method 2)
# ---------------------------------------------------------------------------------------
def _join_same(idx, oracle, ot, qs, k, targets, alpha, pvf, method, use_tl, what):
    gi, gd, git = idx.knn_join(qs, k, targets, alpha, pvf, method, use_target_lists=use_tl, confidence=wi.JOIN_CONF)
    exp, eit = oracle.ivpq_search_in(ot, qs, k, targets, alpha, pvf, method, use_target_lists=use_tl, confidence=wi.JOIN_CONF)
    assert git == eit, (what, git, eit)
    util.assert_same_lists(gi, gd, exp, what)
    return gi, git


@pytest.mark.parametrize("k", wi.JOIN_K)
def test_knn_join_query_kernel_methods_0_and_1(pins, oracle, k):
    """64 cells (two codewords of each half copies of others), 6000 rows, 3000 known targets, 12 queries.  join_lds_bytes is
    far inside the limit at this shape for every width (8 x 16 table entries)."""
    idx, ot = pins("ivpq", (wi.JOIN_QUERY_KC, True))
    qs = wi.join_queries()
    for method in (0, 1):
        for use_tl in (True, False):
            _join_same(idx, oracle, ot, qs, k, wi.join_targets(), wi.JOIN_ALPHA, 4, method, use_tl, f"join method={method} tl={use_tl} k={k}")


@pytest.mark.parametrize("k,pvf", wi.JOIN_PV)
def test_knn_join_query_kernel_post_verification(pins, oracle, k, pvf):
    idx, ot = pins("ivpq", (wi.JOIN_QUERY_KC, True))
    qs = wi.join_queries()
    alpha = wi.join_pv_alpha(pvf)                     # (a round's candidates outnumber the k pvf keys kept: test_width_inputs_cpu.py)
    for use_tl in (True, False):
        _join_same(idx, oracle, ot, qs, k, wi.join_targets(), alpha, pvf, 2, use_tl, f"join method=2 tl={use_tl} k={k} pvf={pvf} alpha={alpha}")


def test_knn_join_fewer_targets_than_k(pins, oracle):
    """20 targets, k = 64: V = 2 (methods 0, 1) and V = 4 (k pvf = 256); the lists end in the reference's padding."""
    idx, ot = pins("ivpq", (wi.JOIN_QUERY_KC, True))
    c = wi.JOIN_FEW
    for method in (0, 1, 2):
        gi, _ = _join_same(idx, oracle, ot, wi.join_queries(), c["k"], wi.join_few_targets(), c["alpha"], c["pvf"], method, True, f"join over 20 targets method={method}")
        assert (gi[:, 20:] == -1).all() and (gi[:, :20] >= 0).all(), method


# ---------------------------------------------------------------------------------------
# F. kNN-join, side sort: side_sort_kernel<V>, L = coarse_codes.  More than 1024 cells: the sorted sides feed the host heap.
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", wi.SIDE_KC)
def test_knn_join_side_sort(gpu, oracle, kc):
    qs = wi.join_queries()
    c = wi.SIDE_CALL
    with _pinned_ivpq(gpu, oracle, wi.ivpq_table(kc, True)) as (idx, ot):
        for method in (0, 1, 2):
            _join_same(idx, oracle, ot, qs, c["k"], wi.join_targets(), c["alpha"], c["pvf"], method, True, f"side sort coarse_codes={kc} method={method}")
            assert idx.last_track()["host_traversals"] >= qs.shape[0], kc      # (every traversal went through the sorted sides)
        _join_same(idx, oracle, ot, qs, c["k"], wi.join_targets(), c["alpha"], c["pvf"], 0, False, f"side sort coarse_codes={kc} no target lists")
        if kc == wi.SIDE_FEW:
            gi, _ = _join_same(idx, oracle, ot, qs, 3 * c["k"], wi.join_few_targets(), 1, c["pvf"], 0, True, f"side sort coarse_codes={kc}, 20 targets")
            assert (gi[:, 20:] == -1).all() and (gi[:, :20] >= 0).all()


def test_knn_join_beyond_1024_coarse_codes_is_refused(gpu, oracle):
    with _pinned_ivpq(gpu, oracle, wi.ivpq_table(1025, False)) as (idx, _):
        with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*coarse_codes=1025"):
            idx.knn_join(wi.join_queries(), 5, wi.join_targets(), 3, 4, 0)


# ---------------------------------------------------------------------------------------
# G. kNN-join, device traversal: join_traverse_kernel<V[, SMALL]>, L = cells = coarse_codes^2
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", wi.TRAVERSE_KC)
def test_knn_join_device_traversal(gpu, oracle, kc):
    """Per width three calls (test_width_inputs_cpu.py restates the rule and measures the stops with the oracle): one that takes
    the SMALL kernel, one that takes the full kernel and stops within the 64 nearest cells, and a deep one whose stops lie
    beyond 63 cells, where the full kernel sorts all 64 V keys and walks the chunks behind the first.  The device hands a query
    to the host heap only for equal keys among the cells it takes, so the host traversals of a call are bounded by its rounds
    times the queries that have equal keys at all -- none, for most tables: the device answered every (query, round) itself.
    Option join_host_traversal = 1 gives the same lists.  Over 20 targets, fewer than k, the lists end in padding."""
    qs = wi.join_queries()
    targets = wi.join_targets()
    tied = qs.shape[0] - len(wi.tie_free_queries(oracle, kc))
    with _pinned_ivpq(gpu, oracle, wi.ivpq_table(kc, False)) as (idx, ot):
        for k, alpha in wi.traverse_calls(kc):
            small = wi.traverse_small(k, alpha, targets.size, kc * kc)
            for method in (0, 1):
                what = f"traversal coarse_codes={kc} k={k} alpha={alpha} small={small} method={method}"
                gi, rounds = _join_same(idx, oracle, ot, qs, k, targets, alpha, 4, method, True, what)
                handed_back = idx.last_track()["host_traversals"]
                assert handed_back <= rounds * tied < qs.shape[0], (what, handed_back, rounds, tied)
                with _option(idx, "join_host_traversal", 1, 0):
                    gh, _ = _join_same(idx, oracle, ot, qs, k, targets, alpha, 4, method, True, what + " on the host")
                    assert idx.last_track()["host_traversals"] >= qs.shape[0], what
                assert np.array_equal(gi, gh), what
        c = wi.JOIN_FEW
        gi, _ = _join_same(idx, oracle, ot, qs, c["k"], wi.join_few_targets(), c["alpha"], c["pvf"], 0, True, f"traversal coarse_codes={kc} over 20 targets")
        assert (gi[:, 20:] == -1).all() and (gi[:, :20] >= 0).all(), kc
