"""-m gpu: every launch whose grid comes from the handle's CU count, with FEWER workgroups than work (option grid_cus; csrc/grid_plan.h).

At the shapes of the rest of the suite `work` is the smaller side of every min(work, f(n_cus)): each workgroup or wave takes one
piece and leaves.  Here the option shrinks n_cus to 1, 2, 3 and 7, so the grid-stride loops, the work counters and the units
dealt round G workgroups go round a second time and more -- with the LDS state of the entry before, the prefetched next record, a
threshold that moved, a ragged last range.  tests/grid_inputs.py lists the cases with their sizes and tests/test_grid_inputs_cpu.py
proves on the CPU that at these sizes the grid IS smaller than the work.

Every case compares ids, ranks and distance / similarity bits with the CPU oracle (or the numpy model of its entry point) and bit
for bit with the same handle at grid_cus = 0; where the value changes the path, the handle's profile names the kernel."""
import numpy as np
import pytest

import grid_inputs as gi
import util

pytestmark = pytest.mark.gpu

CUS = gi.GRID_CUS


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    """(result of call(), names of the kernels it launched)"""
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


def _bits(a, b, what):
    """two (ids, values) results: ids and the values' bits"""
    assert np.array_equal(a[0], b[0]), (what, "ids differ from those at grid_cus = 0")
    u = np.uint32 if a[1].dtype == np.float32 else np.uint64
    assert np.array_equal(a[1].view(u), b[1].view(u)), (what, "float bits differ from those at grid_cus = 0")


def _over_cus(idx, call, check, what, cus=CUS, setters=None):
    """call() at grid_cus = 0, then at every value of `cus`: check(result, names, what) for each, and the same bits as at 0.
    setters: the handles the option is set on (default: idx).  The handle is left at 0."""
    setters = setters or [idx]
    for h in setters:
        h.set_option("grid_cus", 0)
    base, names = _profiled(idx, call)
    check(base, names, f"{what} grid_cus=0")
    for n in cus:
        for h in setters:
            h.set_option("grid_cus", n)
        got, names = _profiled(idx, call)
        check(got, names, f"{what} grid_cus={n}")
        _bits(got, base, f"{what} grid_cus={n}")
    for h in setters:
        h.set_option("grid_cus", 0)
    return base


# =======================================================================================
# a, b (forced), c. IVFADC batches: the filter scan, the item-wise scan, the reference-arithmetic scan
# =======================================================================================
IVF_CALLS = ((5, 0, 1000.0), (32, 0, 1000.0), (5, 1, 100.0))          # (k, found rule, sentinel); W = 3


@pytest.fixture(scope="module")
def ivf(gpu, oracle):
    """K -> (tables, oracle table, handle with fused = 1, the 64 queries); built on first use, 20 000 rows in 32 cells"""
    made = {}

    def get(K):
        if K not in made:
            a = gi.IVF
            t = util.ivf_tables(N=a["N"], C=a["C"], K=K)
            ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
            idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
            idx.set_option("fused", 1)              # (192 items: below the 256 from which a batch takes the cell-grouped scans by itself)
            made[K] = (t, ot, idx, util.queries_from_corpus(a["N"], a["Q"], seed=7)[1])
        return made[K]
    yield get
    for _, _, idx, _ in made.values():
        idx.close()


_EXPECTED = {}   # the oracle's lists of a (table, call): computed once, shared, never written to


def _ivf_expected(oracle, ot, K, qs, k, W, rule, sent, tag=""):
    key = (K, k, W, rule, sent, tag)
    if key not in _EXPECTED:
        _EXPECTED[key] = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
    return _EXPECTED[key]


def _reset(idx):
    for name, v in (("fused", 1), ("fused_kernel", 5), ("codes_u8", 1), ("sparse_items", 2), ("running_bound", 1), ("check_brackets", 0),
                    ("scan_share", 0), ("scan_elastic", 0), ("grid_cus", 0)):
        idx.set_option(name, v)


@pytest.mark.parametrize("K,u8", [(1024, 1), (256, 1), (256, 2), (256, 0)])
def test_filter_scan(ivf, oracle, K, u8):
    """a. 64 queries x 3 probes over 32 cells: at least 12 work entries for 1 .. 7 workgroups.  K = 1024: the six-phase kernel;
    K = 256: the whole-slab kernel (codes_u8 = 1), the six-phase kernel on bytes (2) and on int16 codes (0).  Found rules 0 and 1,
    k = 5 and 32."""
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    idx.set_option("codes_u8", u8)
    W = gi.IVF["W"]
    for k, rule, sent in IVF_CALLS:
        exp = _ivf_expected(oracle, ot, K, qs, k, W, rule, sent)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "ivf_filter" in names and "sparse_items" not in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"filter scan K={K} codes_u8={u8} k={k} rule={rule}")
    assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K,u8", [(1024, 1), (256, 1), (256, 2), (256, 0)])
def test_filter_scan_every_row_refined(ivf, oracle, K, u8):
    """a. running_bound = 1 and check_brackets = 1: the scan keeps every probed row whichever workgroup took its entry, the merge
    refines every one -- bound_checked grows by exactly the rows scanned, no bracket is violated."""
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    idx.set_option("codes_u8", u8)
    idx.set_option("check_brackets", 1)
    W = gi.IVF["W"]
    exp = _ivf_expected(oracle, ot, K, qs, 5, W, 0, 1000.0)
    for n in (0,) + CUS:
        idx.set_option("grid_cus", n)
        before = idx.bound_checked()
        gi_, gd = idx.search(qs, 5, W, sentinel=1000.0, found_rule=0)
        checked, rows = idx.bound_checked() - before, idx.last_scanned_rows()
        util.assert_same_lists(gi_, gd, exp, f"every row K={K} codes_u8={u8} grid_cus={n}")
        assert checked == rows > 0, f"K={K} codes_u8={u8} grid_cus={n}: {checked} brackets checked, {rows} rows scanned"
        assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K", [1024, 256])
def test_filter_scan_sentinel_and_second_round(ivf, oracle, K):
    """a. A sentinel in the middle of the distances (rows whose bracket straddles it are decided by the exact stage; under the
    batch rule the accepted rows decide who probes again): some query of the batch needs a second probing round, whose scan again
    has more entries than workgroups."""
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    W, k = gi.IVF["W"], 5
    d = _ivf_expected(oracle, ot, K, qs, k, W, 0, 1000.0)["dist"].reshape(len(qs), k)
    sent = float(np.median(d[:, k - 1]))
    for rule in (0, 1):
        exp, found, rounds = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule, max_rounds=0)
        if rule == 1:   # (rule 0 counts the rows of the probed lists: one round here; rule 1 the rows below the sentinel)
            assert rounds.max() >= 2 and (rounds == 1).any(), ("input: no query went into a second round, or all did", rounds)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "ivf_filter" in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"sentinel {sent!r} K={K} rule={rule}")
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("K", [1024, 256])
def test_filter_scan_share_4_on_three_cus(ivf, oracle, K):
    """a. scan_share = 4 with grid_cus = 3: n_cus / share is 0, scan_cus takes its min(n_cus, 32) arm -- three workgroups."""
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    idx.set_option("scan_share", 4)
    W = gi.IVF["W"]
    for k, rule, sent in IVF_CALLS:
        exp = _ivf_expected(oracle, ot, K, qs, k, W, rule, sent)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "ivf_filter" in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"scan_share 4 K={K} k={k} rule={rule}", cus=(3,))
    assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K,u8", [(1024, 1), (256, 0)])
def test_filter_scan_two_streams_elastic(ivf, oracle, K, u8):
    """a. freddy_gpu_ivfadc_search_dev on two streams with scan_share = 2 and scan_elastic = 1 (the six-phase kernel's elastic
    instantiation): with so few CUs the cap of scan workgroups is negative -- the grid holds the guaranteed workgroups alone, no
    extra starts, and the advisory words are back at 0.  Round-one lists, final for every query that found k rows."""
    import torch
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    idx.set_option("codes_u8", u8)
    idx.set_option("scan_share", 2)
    idx.set_option("scan_elastic", 1)
    dev = torch.device("cuda", 0)
    W, k, Q = gi.IVF["W"], 5, len(qs)
    batches = [qs, np.ascontiguousarray(qs[::-1] * np.float32(1.01))]
    exp = [oracle.ivfadc_search_many(ot, q, k, W, sentinel=1000.0, found_rule=0) for q in batches]
    first = [oracle.ivfadc_search_many(ot, q, k, W, sentinel=1000.0, found_rule=0, max_rounds=1) for q in batches]
    dq = [torch.from_numpy(q).to(dev) for q in batches]
    res = [torch.zeros((2, Q, k), dtype=torch.int32, device=dev) for _ in batches]
    st = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in batches]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    base = None
    for n in (0,) + CUS:
        idx.set_option("grid_cus", n)
        torch.cuda.synchronize(dev)
        before = idx.scan_elastic_stats()
        for _ in range(3):
            for i in (0, 1):
                with torch.cuda.stream(streams[i]):
                    res[i].zero_()
                    st[i].zero_()
                    idx.search_dev(dq[i].data_ptr(), Q, k, W, 1000.0, 0, res[i][0].data_ptr(), res[i][1].data_ptr(), st[i].data_ptr(),
                                   streams[i].cuda_stream)
        torch.cuda.synchronize(dev)
        after = idx.scan_elastic_stats()
        got = [(r[0].cpu().numpy(), r[1].view(torch.float32).cpu().numpy()) for r in res]
        for i in (0, 1):
            what = f"two streams K={K} codes_u8={u8} grid_cus={n} stream {i}"
            one, found, _ = first[i]
            util.assert_same_lists(got[i][0], got[i][1], one, what + ": round-one lists")
            fin = found >= k
            util.assert_same_lists(got[i][0][fin], got[i][1][fin], {"id": exp[i]["id"][fin], "dist": exp[i]["dist"][fin]}, what + ": finished queries")
            assert (int(st[i][0].item()) != 0) == bool((~fin).any()), what
        assert after["active"] == 0 and after["pending"] == 0, (n, after)
        if n:
            assert gi.plan("cap", n, 64, 0, 2) < 0 and after["started"] == before["started"], (n, before, after)
            for i in (0, 1):
                _bits(got[i], base[i], f"two streams K={K} grid_cus={n} stream {i}")
        else:
            base = got
    assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K", [1024, 256])
def test_reference_arithmetic_scan(ivf, oracle, K):
    """c. fused_kernel = 3 (fused3.h): one persistent workgroup per CU of the handle over at least 16 entries of 12 items."""
    t, ot, idx, qs = ivf(K)
    _reset(idx)
    idx.set_option("fused_kernel", 3)
    W = gi.IVF["W"]
    for k, rule, sent in IVF_CALLS:
        exp = _ivf_expected(oracle, ot, K, qs, k, W, rule, sent)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "ivf_exact_scan" in names and "ivf_filter" not in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"spec2 K={K} k={k} rule={rule}")
    _reset(idx)


# ---- b. the item-wise scan ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse(gpu, oracle):
    t = gi.sparse_tables()
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx.set_option("fused", 1)
    yield t, ot, idx, gi.sparse_queries()
    idx.close()


def test_item_wise_scan_forced(sparse, oracle):
    """b. sparse_items = -2 on 200 cells, 16 queries x 3 probes: 43 thin cells (tests/test_grid_inputs_cpu.py counts them) for 3, 6
    and 9 workgroups of the pair kernel; the work counter deals out the units beyond the first gridDim.x.  Cells of fewer than k
    rows: further probing rounds."""
    t, ot, idx, qs = sparse
    _reset(idx)
    idx.set_option("sparse_items", -2)
    W = gi.SPARSE["W"]
    for k, rule, sent in IVF_CALLS:
        exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "sparse_items" in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"item-wise forced k={k} rule={rule}")
    idx.set_option("check_brackets", 1)
    for n in (0, 1, 3):
        idx.set_option("grid_cus", n)
        before = idx.bound_checked()
        got = idx.search(qs, 5, W, sentinel=1000.0, found_rule=0)
        util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(ot, qs, 5, W, sentinel=1000.0, found_rule=0), f"item-wise, every row, grid_cus={n}")
        assert idx.bound_checked() - before == idx.last_scanned_rows() > 0, n
    assert idx.bound_violations() == 0
    _reset(idx)


def test_item_wise_scan_by_its_own_rule(sparse, oracle):
    """b. 48 items on 200 cells: fewer than four items per cell, and 48 >= 16 n_cus for n_cus <= 3 -- the batch takes the item-wise
    scan by itself at grid_cus 1, 2, 3 and not at 7 or 0.  The same lists either way."""
    t, ot, idx, qs = sparse
    _reset(idx)
    W = gi.SPARSE["W"]
    for k, rule, sent in IVF_CALLS:
        exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            n = int(what.rsplit("=", 1)[1])
            assert ("sparse_items" in names) == (1 <= n <= 3), (what, sorted(names))
            assert "ivf_filter" in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"item-wise unforced k={k} rule={rule}")
    assert idx.bound_violations() == 0


# =======================================================================================
# d. the multi scan (multi.h): the shapes the filter scan is not built for
# =======================================================================================
@pytest.mark.parametrize("key", list(gi.MULTI))
def test_multi_scan(gpu, oracle, key):
    """d. 25-d, m = 5, K = 256 and m = 30, K = 32: ivf_multi_kernel's entries of 8 items, at least 24 of them for two workgroups
    per CU of the handle."""
    s = gi.MULTI[key]
    t = util.shape_ivf_tables(s["d"], s["m"], s["K"], s["C"], s["N"])
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx.set_option("fused", 1)
    qs = util.shape_queries(s["N"], s["d"], s["Q"], seed=3)
    for k, rule, sent in IVF_CALLS:
        exp = oracle.ivfadc_search_many(ot, qs, k, s["W"], sentinel=sent, found_rule=rule)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert "ivf_multi_scan" in names and "ivf_filter" not in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, s["W"], sentinel=sent, found_rule=rule), check, f"multi {key} k={k} rule={rule}")
    idx.close()


# =======================================================================================
# e. the flat PQ table through the cell-grouped scan
# =======================================================================================
@pytest.fixture(scope="module")
def pq(gpu, oracle):
    t = util.pq_tables(N=gi.PQ["N"], K=256)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    yield t, ot, idx, util.queries_from_corpus(gi.PQ["N"], 64, seed=21)[1]
    idx.close()


@pytest.mark.parametrize("Q", [16, 64])
def test_pq_batch_over_pseudo_lists(pq, oracle, Q):
    """e. pq_fused = 1 on 20 000 rows: five pseudo-lists, ceil(Q / 16) entries each (5 and 20) for 1 .. 7 workgroups of the view's
    filter scan -- the option set on the owner reaches its view; pq_fused = 0: the generic kernels."""
    t, ot, idx, qs = pq
    qs = qs[:Q].copy()
    qs[7] *= np.float32(20.0)                         # farther than the sentinel from everything: the empty list
    for k in (5, 32):
        exp = np.stack([oracle.pq_search(ot, q, k) for q in qs])
        for fused in (1, 0):
            idx.set_option("pq_fused", fused)

            def check(got, names, what):
                util.assert_same_lists(got[0], got[1], exp, what)
                assert ("pq_front" in names and "ivf_filter" in names) == (fused == 1) and ("adc_scan" in names) == (fused == 0), (what, sorted(names))
            _over_cus(idx, lambda: idx.search(qs, k, sentinel=100.0), check, f"pq batch Q={Q} k={k} pq_fused={fused}")
    idx.set_option("pq_fused", -1)
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("Q", [16, 64])
def test_pq_subset_batch_over_the_sub_view(pq, oracle, Q):
    """e. the same with subset_ids: 9 000 rows gathered into a view of their own (three pseudo-lists), refreshed by every call."""
    t, ot, idx, qs = pq
    qs = qs[:Q]
    rng = np.random.default_rng(5)
    targets = rng.choice(np.arange(1, gi.PQ["N"] + 1), size=9000, replace=False).astype(np.int32)
    targets = np.concatenate([targets, targets[:40], np.array([gi.PQ["N"] + 9, -2], np.int32)])
    exp = oracle.pq_search_in_batch(ot, qs, 5, targets, use_target_lists=True)
    for fused in (1, 0):
        idx.set_option("pq_fused", fused)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            assert ("pq_front" in names) == (fused == 1), (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, 5, sentinel=1000.0, subset_ids=targets), check, f"pq subset Q={Q} pq_fused={fused}")
    idx.set_option("pq_fused", -1)
    assert idx.bound_violations() == 0


# =======================================================================================
# f. one launch (one.h)
# =======================================================================================
def test_ivf_one_launch_with_few_workgroups(ivf, oracle):
    """f. ivf_one_kernel with G = 3, 7 and 13 workgroups: W * 12 = 36 table units dealt round them (n_slot = 1), ceil(32 / G)
    cells per workgroup in the coarse stage, G / W parts per item (a workgroup without an item at G = 7 and 13).  At grid_cus = 2,
    G < W: the multi-launch path answers, with the same list; W = 7 moves that edge to G = 7 (one workgroup per item) and 13 (six
    without an item).  After each, a call at grid_cus = 0 is still one launch."""
    t, ot, idx, qs = ivf(256)
    _reset(idx)
    idx.set_option("fused", -1)
    for k, W, rule, sent in ((5, gi.ONE_IVF["W"], 0, 1000.0), (32, gi.ONE_IVF["W"], 0, 1000.0), (5, gi.ONE_IVF["W"], 1, 100.0), (5, 7, 0, 1000.0)):
        for qi in (0, 9, 33):
            q = qs[qi:qi + 1]
            exp = oracle.ivfadc_search(ot, q[0], k, W, sentinel=sent, found_rule=rule)[None]
            idx.set_option("grid_cus", 0)
            base, names = _profiled(idx, lambda: idx.search(q, k, W, sentinel=sent, found_rule=rule))
            util.assert_same_lists(base[0], base[1], exp, f"ivf_one k={k} W={W} rule={rule} query {qi}")
            assert "ivf_one" in names, sorted(names)
            for n in (2, 3, 7, 13):
                what = f"ivf_one k={k} W={W} rule={rule} query {qi} grid_cus={n}"
                idx.set_option("grid_cus", n)
                got, names = _profiled(idx, lambda: idx.search(q, k, W, sentinel=sent, found_rule=rule))
                util.assert_same_lists(got[0], got[1], exp, what)
                _bits(got, base, what)
                assert ("ivf_one" in names) == (n >= W), (what, sorted(names))
                assert n >= W or "adc_scan" in names or "ivf_filter" in names, (what, sorted(names))
                idx.set_option("grid_cus", 0)
                again, names = _profiled(idx, lambda: idx.search(q, k, W, sentinel=sent, found_rule=rule))
                assert "ivf_one" in names, (what, "the handle switched one launch off", sorted(names))
                _bits(again, base, what + ", back at 0")
    _reset(idx)


def test_ivf_one_launch_lds_fallback(gpu, oracle):
    """f. 4 096 cells at grid_cus = 3: a workgroup's 1 366 centroid rows do not fit the LDS, the host takes the multi-launch path
    before any launch; at grid_cus = 0 (16 rows per workgroup) the same query is one launch.  Random tables: about five rows per cell."""
    s = gi.ONE_IVF_WIDE
    rng = np.random.default_rng(41)
    N, C, K = s["N"], s["C"], s["K"]
    coarse = rng.standard_normal((C, 300)).astype(np.float32) * np.float32(0.3)
    codebook = (rng.standard_normal((12, K, 25)) * 0.1).astype(np.float32)
    cell = np.sort(rng.integers(0, C, size=N))
    codes = rng.integers(0, K, size=(N, 12)).astype(np.int16)
    list_off = np.zeros(C + 1, np.int32)
    list_off[1:] = np.cumsum(np.bincount(cell, minlength=C))
    ids = (np.arange(N) * 3 + 2).astype(np.int32)
    ot = oracle.ivf_table(coarse, codebook, list_off, ids, codes)
    idx = gpu.IVFIndex(coarse, codebook, list_off, ids, codes)
    qs = (coarse[rng.integers(0, C, size=6)] + 0.02 * rng.standard_normal((6, 300))).astype(np.float32)
    for qi, q in enumerate(qs):
        for k, W in ((5, 3), (2, 3)):
            exp = oracle.ivfadc_search(ot, q, k, W, sentinel=1000.0, found_rule=0)[None]
            idx.set_option("grid_cus", 0)
            base, names = _profiled(idx, lambda: idx.search(q[None], k, W))
            util.assert_same_lists(base[0], base[1], exp, f"4096 cells query {qi} k={k}")
            assert "ivf_one" in names, sorted(names)
            idx.set_option("grid_cus", 3)
            got, names = _profiled(idx, lambda: idx.search(q[None], k, W))
            util.assert_same_lists(got[0], got[1], exp, f"4096 cells query {qi} k={k} grid_cus=3")
            _bits(got, base, f"4096 cells query {qi} k={k} grid_cus=3")
            assert "ivf_one" not in names and names, sorted(names)
    idx.set_option("grid_cus", 0)
    _, names = _profiled(idx, lambda: idx.search(qs[:1], 5, 3))
    assert "ivf_one" in names, sorted(names)
    idx.close()


def test_pq_one_launch_with_few_workgroups(gpu, oracle):
    """f. pq_one_kernel on 5 000 rows (79 row blocks) with G = 1, 2, 3 and 7 workgroups: 12 table units dealt round them, 79 / G
    blocks each -- at G = 1 a wave's ring of eight blocks goes round twice.  After each, a call at grid_cus = 0 is one launch."""
    n = gi.ONE_PQ["N"]
    t = util.pq_tables(N=20000, K=gi.ONE_PQ["K"])
    ids, codes = t["ids"][:n], t["codes"][:n].copy()
    codes[1000:1100] = codes[999]                     # equal distances: the order is the scan position's
    ot = oracle.pq_table(t["codebook"], ids, codes)
    idx = gpu.PQIndex(t["codebook"], ids, codes)
    _, qs = util.queries_from_corpus(n, 6, seed=5)
    qs[3] *= np.float32(20.0)
    for k in (5, 32):
        for qi, q in enumerate(qs):
            exp = oracle.pq_search(ot, q, k)[None]

            def check(got, names, what):
                util.assert_same_lists(got[0], got[1], exp, what)
                assert "pq_one" in names, (what, sorted(names))
            _over_cus(idx, lambda: idx.search(q[None], k, sentinel=100.0), check, f"pq_one k={k} query {qi}")
            _, names = _profiled(idx, lambda: idx.search(q[None], k, sentinel=100.0))
            assert "pq_one" in names, ("the handle switched one launch off", sorted(names))
    idx.close()


# =======================================================================================
# g. exact kNN: filter + refine, and the all-exact scan
# =======================================================================================
def _exact_table(d, N, scale=1.0):
    """tests/test_gpu_shapes.py _exact_table: duplicate rows at 100 .. 139 and N / 2 .. N / 2 + 39, 70 queries"""
    x = (util.shape_corpus(N, d).numpy() * np.float32(scale)).astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::N // 70][:70].copy()
    qs[3] = -qs[3]
    qs[6] = x[100]
    return x, ids, qs


@pytest.fixture(scope="module")
def exact(gpu, oracle):
    made = {}

    def get(d):
        if d not in made:
            N = gi.EXACT["N"]
            x, ids, qs = _exact_table(d, N)
            made[d] = (x, ids, qs, [oracle.exact_knn(x, ids, q, 32) for q in qs], gpu.VectorIndex(ids, x))
        return made[d]
    yield get
    for *_, idx in made.values():
        idx.close()


@pytest.mark.parametrize("d", [64, 100])
def test_exact_knn_filter_strip_loop(exact, d):
    """g. 8 232 rows = 258 strips of 32: at grid_cus = 1 two workgroups, 16 strips and more per wave (at the device's count 264
    waves: one each).  The duplicate rows at N / 2 sit in strips 128 and 129, which only a later iteration reaches; their copies in
    strips 3 and 4 are read by the first."""
    x, ids, qs, exp, idx = exact(d)
    idx.set_option("check_brackets", 0)
    idx.set_option("exact_filter", 1)
    for Q in (1, 9, 70):
        for k in (1, 5, 32):
            def check(got, names, what):
                util.assert_exact_lists(got[0], got[1], exp, k, what)
                assert "exact_filter" in names and "exact_refine" in names, (what, sorted(names))
            _over_cus(idx, lambda: idx.search(qs[:Q], k), check, f"exact d={d} Q={Q} k={k}")
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("d", [64, 100])
def test_exact_knn_every_row_refined(exact, d):
    """g. check_brackets = 4: every (query, row) pair is a candidate whichever iteration of the strip loop read it --
    bound_checked grows by Q * N, no violation."""
    x, ids, qs, exp, idx = exact(d)
    idx.set_option("exact_filter", 1)
    idx.set_option("check_brackets", 4)
    N = gi.EXACT["N"]
    for n in (0,) + CUS:
        idx.set_option("grid_cus", n)
        before = idx.bound_checked()
        got, names = _profiled(idx, lambda: idx.search(qs[:9], 5))
        util.assert_exact_lists(got[0], got[1], exp, 5, f"every row d={d} grid_cus={n}")
        assert "exact_filter" in names, sorted(names)
        assert idx.bound_checked() - before == 9 * N, (n, idx.bound_checked() - before)
        assert idx.bound_violations() == 0
    idx.set_option("check_brackets", 0)
    idx.set_option("grid_cus", 0)


def test_exact_knn_all_exact_scan(exact):
    """g. exact_filter = 0: exact_scan_kernel (its grid does not come from the CU count; the option must not reach it)."""
    x, ids, qs, exp, idx = exact(64)
    idx.set_option("exact_filter", 0)
    for Q, k in ((9, 5), (70, 32)):
        def check(got, names, what):
            util.assert_exact_lists(got[0], got[1], exp, k, what)
            assert "exact_scan" in names and "exact_filter" not in names, (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs[:Q], k), check, f"exact scan Q={Q} k={k}")
    idx.set_option("exact_filter", 1)


# =======================================================================================
# h. exact analogies
# =======================================================================================
@pytest.mark.parametrize("method", ["3cosadd", "3cosmul", "pair_direction"])
def test_exact_analogies(gpu, method):
    """h. 8 232 x 300 with the filter forced: an_filter_kernel<1> (3CosAdd) and <3> (3CosMul) walk 258 strips with 2 .. 14
    workgroups; pair direction (no filter: the all-exact kernels) on the un-normalised table.  40 analogies: a pass of 32 and one
    of 8; ids and score bits of the numpy models."""
    import analogy_model as am
    import pair_model as pm
    N = gi.EXACT["N"]
    x = util.corpus(N).numpy().copy()
    if method == "pair_direction":
        x = x * np.random.default_rng(5).uniform(0.5, 4.0, size=(N, 1)).astype(np.float32)
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    rng = np.random.default_rng(3)
    t = rng.integers(0, N, size=(40, 3))
    t[:4] = rng.integers(0, 32, size=(4, 3))
    t[4] = (7, 7, 123)
    x[N - 100] = x[123]                               # the copy of v3, in a strip of the last iterations
    t[5] = (9, N // 2, 9)
    triples = ids[t]
    x_t = np.ascontiguousarray(x.T)
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_filter", 1)
    for k in (1, 5, 32):
        exp = pm.model(x, ids, triples, k, x_t=x_t) if method == "pair_direction" else am.model(x, ids, triples, k, method, x_t=x_t)

        def check(got, names, what):
            assert np.array_equal(got[0], exp[0]), (what, np.nonzero((got[0] != exp[0]).any(1))[0][:5])
            assert np.array_equal(got[1].view(np.uint64), exp[1].view(np.uint64)), what
            if method == "pair_direction":
                assert "analogy_pair_scan" in names and "analogy_filter" not in names, (what, sorted(names))
            else:
                assert "analogy_filter" in names, (what, sorted(names))
                st = idx.last_analogy_stats()
                assert st["filter_passes"] == 2 and st["redone_passes"] == 0, (what, st)
        _over_cus(idx, lambda: idx.analogy(triples, k=k, method=method), check, f"analogy {method} k={k}")
    if method != "pair_direction":
        idx.set_option("check_brackets", 8)           # every row refined for every analogy
        for n in (0, 1):
            idx.set_option("grid_cus", n)
            c0 = idx.bound_checked()
            got = idx.analogy(triples[:9], k=5, method=method)
            exp = am.model(x, ids, triples[:9], 5, method, x_t=x_t)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint64), exp[1].view(np.uint64)), n
            assert idx.bound_checked() - c0 == 9 * N, (n, idx.bound_checked() - c0)
    assert idx.bound_violations() == 0
    idx.close()


# =======================================================================================
# i. the exact join
# =======================================================================================
def test_exact_join_strip_chunks(gpu, oracle):
    """i. 8 200 known targets = 33 steps of 256 rows for gx = 5 .. 14 workgroups per query tile (33 at the device's count).
    Q = 70 (one tile of 128 or two of 64) and Q = 200 (two or four), exact_join_tile 0 and 64."""
    N, d = 20000, 300
    x = util.shape_corpus(N, d).numpy().astype(np.float32).copy()
    x[N // 2:N // 2 + 40] = x[100:140]
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::N // 200][:200].copy()
    qs[3] = -qs[3]
    qs[6] = x[100]
    rng = np.random.default_rng(2)
    both = np.concatenate([np.arange(100, 120), np.arange(N // 2, N // 2 + 20)])
    rows = np.concatenate([both, rng.choice(np.setdiff1d(np.arange(N), both), gi.JOIN["targets"] - both.size, replace=False)])
    targets = rng.permutation(np.concatenate([ids[rows], ids[rows[:60]], np.array([4, 10**8, -7], np.int32)])).astype(np.int32)
    exp = [oracle.exact_knn(x, ids, q, 32, targets) for q in qs]
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_filter", 1)
    for tile in (0, 64):
        idx.set_option("exact_join_tile", tile)
        for Q, k in ((70, 5), (200, 32), (200, 1)):
            def check(got, names, what):
                util.assert_exact_lists(got[0], got[1], exp, k, what)
                assert "exact_join_filter" in names and "exact_join_refine" in names, (what, sorted(names))
                st = idx.last_join_stats()
                assert st["redone_queries"] == 0 and st["filter_queries"] == Q, (what, st)
            _over_cus(idx, lambda: idx.join(qs[:Q], k, targets), check, f"join Q={Q} k={k} tile={tile}")
    idx.set_option("check_brackets", 4)
    idx.set_option("grid_cus", 1)
    before = idx.bound_checked()
    got = idx.join(qs[:70], 5, targets)
    util.assert_exact_lists(got[0], got[1], exp, 5, "join, every pair, grid_cus=1")
    assert idx.bound_checked() - before == 70 * gi.JOIN["targets"]
    assert idx.bound_violations() == 0
    idx.close()


# =======================================================================================
# j. table statistics under mutation
# =======================================================================================
def test_table_statistics_rows_of_later_iterations(gpu, oracle):
    """j. exf_table_stats_kernel at grid_cus = 1: eight workgroups of four rows, 32 rows per sweep.  The longest row and the
    largest element of an append, of an update and of what a removal leaves sit far behind the first sweep; a statistic that
    missed them would scale the f16 operands wrongly or bound the norms too low -- with check_brackets = 4 every row's bracket
    is compared.  Lists equal the oracle's and, bit for bit, a fresh pin's at the default."""
    d, n0, n_app = 64, gi.STATS["N0"], gi.STATS["append"]
    total = n0 + n_app
    x = util.shape_corpus(total, d).numpy().astype(np.float32).copy()
    ids = (np.arange(total) * 2 + 3).astype(np.int32)
    x[n0 - 37] *= np.float32(9.0)                     # pin: the longest row, row 563 of 600
    x[n0 + n_app - 21] *= np.float32(40.0)            # append: the longest row and the largest element, row 479 of the 500 new
    qs = np.concatenate([x[::97][:9], x[n0 - 37:n0 - 36], x[n0 + n_app - 21:n0 + n_app - 20]]).copy()

    def compare(idx, xs, is_, what):
        fresh = gpu.VectorIndex(is_, xs)
        for h in (idx, fresh):
            h.set_option("exact_filter", 1)
            h.set_option("check_brackets", 4)
        before = idx.bound_checked()
        got, names = _profiled(idx, lambda: idx.search(qs, 5))
        assert "exact_filter" in names, (what, sorted(names))
        util.assert_exact_lists(got[0], got[1], [oracle.exact_knn(xs, is_, q, 5) for q in qs], 5, what)
        _bits(got, fresh.search(qs, 5), what + " (fresh pin)")
        assert idx.bound_checked() - before == len(qs) * len(is_), what
        assert idx.bound_violations() == 0 and fresh.bound_violations() == 0, what
        fresh.close()

    idx = gpu.VectorIndex(ids[:n0], x[:n0])
    idx.set_option("grid_cus", 1)
    compare(idx, x[:n0], ids[:n0], "pinned")
    idx.append_rows(ids[n0:], vectors=x[n0:])
    compare(idx, x, ids, "after the append")
    xs = x.copy()                                     # update: the long rows shrink, another row far down becomes the longest
    at = np.array([n0 - 37, n0 + n_app - 21, total - 5])
    xs[at[:2]] = x[[3, 4]]
    xs[at[2]] = x[5] * np.float32(300.0)
    assert idx.update_rows(ids[at], vectors=xs[at]) == 3
    compare(idx, xs, ids, "after the update")
    gone = np.concatenate([np.arange(0, 40), [total - 5]])      # removal: the statistics are taken again from row 0
    keep = np.setdiff1d(np.arange(total), gone)
    xs[keep[-9]] = xs[keep[-9]] * np.float32(25.0)
    assert idx.update_rows(ids[keep[-9:-8]], vectors=xs[keep[-9:-8]]) == 1
    assert idx.remove_rows(ids[gone]) == gone.size
    compare(idx, xs[keep], ids[keep], "after the removal")
    idx.close()


# =======================================================================================
# k. similarity and assignment
# =======================================================================================
@pytest.mark.parametrize("nb", gi.SIM["nb"])
def test_similarity_ranges_of_tiles(gpu, nb):
    """k. 200 rows of A = 13 tiles of 16 (the last of 8 rows) against nb = 200 / 1 100 rows of B (4 / 18 blocks): at grid_cus = 1
    a workgroup walks 4 / 13 tiles, at 3 two / five with a ragged last range (tests/grid_inputs.py sim_cases); A by ids and by vectors."""
    import similarity_inputs as si
    import similarity_model as sm
    ids, x = si.table(300)
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(nb)
    a = si.draw_ids(ids, gi.SIM["na"], rng)
    b = si.draw_ids(ids, nb, rng)
    a_vec = np.zeros((a.size, 300), np.float32)
    r = sm.rows_of(ids, a)
    a_vec[r >= 0] = x[r[r >= 0]]
    for side, what in ((a, "ids"), (a_vec, "vectors")):
        exp = sm.matrix(ids, x, side, b)
        thr = si.join_threshold(*exp)
        ej = sm.join_of(*exp, thr)
        base = None
        for n in (0,) + CUS:
            vec.set_option("grid_cus", n)
            got, names = _profiled(vec, lambda: vec.similarity_matrix(side, b))
            w = f"similarity A by {what} nb={nb} grid_cus={n}"
            assert sm.same_floats(got[0], exp[0]), w
            assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), w
            assert "sim_matrix_kernel" in names, (w, sorted(names))
            gj = vec.similarity_join(side, b, thr)
            assert gj[3] == ej[3] and np.array_equal(gj[0], ej[0]) and np.array_equal(gj[1], ej[1]) and sm.same_floats(gj[2], ej[2]), w
            if base is None:
                base = got
            assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32)), w
    vec.close()


def test_pq_assign_four_targets_per_thread(gpu, oracle):
    """k. 2 148 targets at grid_cus = 1: assign_pq_kernel's RPT = 4 instantiation (from 2 048 n_cus targets on), three workgroups of
    1 024 targets, the last with 100; RPT = 1 at every other value.  pq_assign and cluster(pq) against their numpy models."""
    import assign_model as am
    import cluster_inputs as ci
    import cluster_model as cm
    x, ids, cb, codes = ci.tables("300d_m12")
    vec, pq = gpu.VectorIndex(ids, x), gpu.PQIndex(cb, ids, codes)
    rng = np.random.default_rng(17)
    n = gi.ASSIGN["targets"]
    cent = np.stack([x[rng.choice(ci.N, 10)].mean(axis=0) for _ in range(17)]).astype(np.float32)
    cent[4] = cent[0]
    targets = rng.choice(ids, n).astype(np.int32)
    targets[5] = ci.N + 7; targets[n - 3] = -4                       # ids without a row, one of them in the ragged tail
    targets[10:20] = np.arange(101, 111); targets[n - 20:n - 10] = np.arange(5001, 5011)   # duplicated rows
    exp = am.pq_assign(oracle, cb, ids, codes, cent, targets)
    tokens = rng.choice(ids, n).astype(np.int32)
    draws = rng.random(cm.n_draws(5, 3))
    exp_c = cm.pq(oracle, ids, x, cb, ids, codes, tokens, 5, draws, 3, sentinel=1000.0)
    for g in (0,) + CUS:
        for h in (vec, pq):
            h.set_option("grid_cus", g)
        got, names = _profiled(pq, lambda: pq.assign(cent, targets))
        assert am.same(got, exp), f"pq_assign grid_cus={g}: {np.flatnonzero(got[0] != exp[0])[:8]}"
        assert "assign_pq_kernel" in names, sorted(names)
        assert cm.same(vec.cluster(tokens, 5, draws, rounds=3, pq=pq), exp_c), f"cluster(pq) grid_cus={g}"
    vec.close(); pq.close()


# =======================================================================================
# l. the option itself
# =======================================================================================
def test_a_value_above_the_device_count_is_clamped(sparse, oracle):
    """l. grid_cus = 100 000: the device's count -- the lists and the kernels of the default (no item-wise scan by itself)."""
    t, ot, idx, qs = sparse
    _reset(idx)
    W = gi.SPARSE["W"]
    exp = oracle.ivfadc_search_many(ot, qs, 5, W)
    base, names0 = _profiled(idx, lambda: idx.search(qs, 5, W))
    for v in (100000, 2 ** 40, -3):
        idx.set_option("grid_cus", v)
        got, names = _profiled(idx, lambda: idx.search(qs, 5, W))
        util.assert_same_lists(got[0], got[1], exp, f"grid_cus={v}")
        _bits(got, base, f"grid_cus={v}")
        assert names == names0 and "sparse_items" not in names, (v, sorted(names), sorted(names0))
    idx.set_option("grid_cus", 0)
    with pytest.raises(Exception, match="unknown option"):
        idx.set_option("grid_cu", 1)


def test_the_option_holds_across_mutations_of_an_ivf_handle(gpu, oracle):
    """l. grid_cus = 2 set once; after append_rows, update_codebook, remove_rows and update_rows the batch of 48 items still takes
    the item-wise scan by itself (n_cus is still 2), with the oracle's lists on the new tables."""
    t = gi.sparse_tables()
    qs, W = gi.sparse_queries(), gi.SPARSE["W"]
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx.set_option("fused", 1)
    idx.set_option("grid_cus", 2)

    def check(tables, what):
        ot = oracle.ivf_table(tables["coarse"], tables["codebook"], tables["list_off"], tables["ids"], tables["codes"])
        got, names = _profiled(idx, lambda: idx.search(qs, 5, W))
        util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(ot, qs, 5, W), what)
        assert "sparse_items" in names, (what, sorted(names))
    check(t, "pinned")
    rng = np.random.default_rng(3)
    C, n_new = gi.SPARSE["C"], 300
    new_ids = (np.arange(n_new) + int(t["ids"].max()) + 1).astype(np.int32)
    new_cell = rng.integers(0, C, n_new).astype(np.int32)
    new_codes = rng.integers(0, gi.SPARSE["K"], (n_new, 12)).astype(np.int16)
    idx.append_rows(new_ids, coarse_id=new_cell, codes=new_codes)
    order = np.argsort(new_cell, kind="stable")
    lo = t["list_off"]
    ids2, codes2, off2 = [], [], [0]
    for c in range(C):
        sel = order[new_cell[order] == c]
        ids2.append(np.concatenate([t["ids"][lo[c]:lo[c + 1]], new_ids[sel]]))
        codes2.append(np.concatenate([t["codes"][lo[c]:lo[c + 1]], new_codes[sel]]))
        off2.append(off2[-1] + len(ids2[-1]))
    t2 = dict(t, list_off=np.array(off2, np.int32), ids=np.concatenate(ids2), codes=np.concatenate(codes2))
    check(t2, "after the append")
    cb = np.array(t["codebook"], np.float32, copy=True)
    cb[:, ::3] += np.float32(0.01) * rng.standard_normal(cb[:, ::3].shape).astype(np.float32)
    idx.update_codebook(cb)
    check(dict(t2, codebook=cb), "after the codebook swap")
    assert idx.remove_rows(new_ids) == n_new                      # back to the pinned rows, under the new codebook
    check(dict(t, codebook=cb), "after the removal")
    at = rng.choice(t["ids"].size, 40, replace=False)             # new codes for 40 rows, each in its own list
    codes3 = t["codes"].copy()
    codes3[at] = rng.integers(0, gi.SPARSE["K"], (at.size, 12)).astype(np.int16)
    cell = (np.searchsorted(lo, at, side="right") - 1).astype(np.int32)
    assert idx.update_rows(t["ids"][at], coarse_id=cell, codes=codes3[at]) == at.size
    check(dict(t, codebook=cb, codes=codes3), "after the update")
    assert idx.bound_violations() == 0
    idx.close()


def test_the_option_reaches_a_pq_handle_across_mutations(gpu, oracle):
    """l. a PQ handle: grid_cus = 1 set BEFORE the view exists, then after it exists; the one-launch kernel, the view's scan and the
    sub-view's give the oracle's lists before and after append_rows (which frees the views: the next ones copy the value)."""
    n = 9000
    t = util.pq_tables(N=20000, K=256)
    ids, codes = t["ids"], t["codes"]
    idx = gpu.PQIndex(t["codebook"], ids[:n], codes[:n])
    idx.set_option("grid_cus", 1)
    idx.set_option("pq_fused", 1)
    _, qs = util.queries_from_corpus(n, 40, seed=21)
    sub = np.random.default_rng(5).choice(ids[:n], size=5000, replace=False).astype(np.int32)

    def check(rows, what):
        ot = oracle.pq_table(t["codebook"], ids[:rows], codes[:rows])
        for g in (1, 2, 0, 1):
            idx.set_option("grid_cus", g)
            got, names = _profiled(idx, lambda: idx.search(qs, 5, sentinel=100.0))
            util.assert_same_lists(got[0], got[1], np.stack([oracle.pq_search(ot, q, 5) for q in qs]), f"{what} grid_cus={g}")
            assert "pq_front" in names, sorted(names)
            got = idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)
            util.assert_same_lists(got[0], got[1], oracle.pq_search_in_batch(ot, qs, 5, sub, use_target_lists=True), f"{what} subset grid_cus={g}")
            idx.set_option("pq_fused", -1)          # (forced, the view's scan answers a single query too)
            got, names = _profiled(idx, lambda: idx.search(qs[:1], 5, sentinel=100.0))
            idx.set_option("pq_fused", 1)
            util.assert_same_lists(got[0], got[1], oracle.pq_search(ot, qs[0], 5)[None], f"{what} one query grid_cus={g}")
            assert "pq_one" in names, sorted(names)
    check(n, "pinned")
    idx.append_rows(ids[n:n + 700], codes=np.ascontiguousarray(codes[n:n + 700]))
    check(n + 700, "after the append")
    assert idx.bound_violations() == 0
    idx.close()


def test_replicas_follow_the_option(gpu, oracle):
    """l. devices = [0, 0]: a host batch is split over the handle and its replica; set_option reaches both (the primary's profile
    shows the item-wise scan its half of the batch takes by itself at grid_cus = 1: 24 items >= 16 n_cus) and the lists are the
    oracle's at every value."""
    t = gi.sparse_tables()
    qs, W = gi.sparse_queries(), gi.SPARSE["W"]
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"], devices=[0, 0])
    assert idx.replicas == 2
    idx.set_option("fused", 1)
    for k, rule, sent in IVF_CALLS:
        exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)

        def check(got, names, what):
            util.assert_same_lists(got[0], got[1], exp, what)
            n = int(what.rsplit("=", 1)[1])
            assert ("sparse_items" in names) == (n == 1), (what, sorted(names))
        _over_cus(idx, lambda: idx.search(qs, k, W, sentinel=sent, found_rule=rule), check, f"replicas k={k} rule={rule}")
    assert idx.bound_violations() == 0
    idx.close()
