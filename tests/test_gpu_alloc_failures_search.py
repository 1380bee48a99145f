"""-m gpu: every allocation of every search and stand-alone call fails once (the allocation seam, csrc/alloc_hook.h) on a freshly
pinned handle with a cold workspace -- the state in which a call allocates most.

A scenario is one call.  It runs once on a cold handle with the seam's counter read around it: A allocations, at least the FLOOR
read off the code (written beside the scenario).  Then for EVERY n in 1 .. A: fresh handles, the n-th allocation from now fails,
the call is made.  What must hold:
  - the call returns FREDDY_E_NOMEM, with a message, and exactly one allocation failed;
  - freddy_gpu_index_bytes of every handle involved is unchanged;
  - the same call made again, nothing armed, returns the expected lists bit for bit -- the oracle's (or the numpy model's built on
    it) for every call, computed once per scenario;
  - after unpin the live allocations (count, bytes, digest) are those of before the pin.
Two more tests: the steady state allocates NOTHING (the structural argument that the seam cannot have moved the headline figure:
with nothing allocated, the only code it added to the timed region is never reached), and one failure that comes from the runtime
itself, after which the very next search is healthy.
Tables: N <= 9000 rows, Q <= 70 queries."""
import ctypes as C

import numpy as np
import pytest

import analogy_model as anm
import approx_analogy_model as aam
import assign_model as asm
import pv_model as pm
import util
from test_gpu_mutation import _exact_same, _vec_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module", autouse=True)
def tracking(gpu):
    gpu.alloc_fail_nth(0)
    gpu.alloc_track(True)
    yield
    gpu.alloc_fail_nth(0)
    gpu.alloc_track(False)


@pytest.fixture(scope="module")
def tabs():
    """the tables every scenario pins: the standard shapes at the sizes the mutation tests use, ids 1 .. N"""
    x = util.corpus(20000).numpy()
    pq, ivf, ivpq = util.pq_tables(), util.ivf_tables(), util.ivpq_tables()
    n_pq, n_ivpq, n_vec = 4200, 3000, 2000
    keep = ivf["ids"] <= 6000                            # the rows with ids 1 .. 6000, list by list
    lo = np.zeros(ivf["list_off"].size, np.int32)
    cell_sorted = np.repeat(np.arange(lo.size - 1), np.diff(ivf["list_off"]))
    lo[1:] = np.cumsum(np.bincount(cell_sorted[keep], minlength=lo.size - 1))
    xv, idv = _vec_table(64, 8300)                       # the exact filter serves from 8192 rows on
    return dict(x=x,
                pq=(pq["codebook"], pq["ids"][:n_pq], pq["codes"][:n_pq]),
                ivf=(ivf["coarse"], ivf["codebook"], lo, ivf["ids"][keep], ivf["codes"][keep]),
                ivpq=(ivpq["codebook"], ivpq["coarse"], ivpq["ids"][:n_ivpq], ivpq["coarse_id"][:n_ivpq], ivpq["codes"][:n_ivpq], ivpq["vectors"][:n_ivpq],
                      ivpq["stats"]),
                vec300=(np.arange(1, n_vec + 1, dtype=np.int32), x[:n_vec]),
                vec64=(idv, xv))


def _live(gpu):
    st = gpu.alloc_stats()
    return st.live, st.live_bytes, st.digest


class Lazy:
    def __init__(self, fn):
        self.fn, self.v = fn, None

    def __call__(self):
        if self.v is None:
            self.v = self.fn()
        return self.v


SUMMARY = []


def _sweep(gpu, name, make, call, check, floor):
    """make() -> list of cold handles; call(handles) -> result; check(result) compares it with the expected lists"""
    s0 = _live(gpu)
    hs = make()
    c0 = gpu.alloc_stats().calls
    res = call(hs)
    A = gpu.alloc_stats().calls - c0
    check(res)
    for h in hs:
        h.close()
    assert _live(gpu) == s0, f"{name}: unpin left allocations behind"
    assert A >= floor, f"{name}: the call made {A} allocations through the seam, the code allocates at least {floor}"
    for n in range(1, A + 1):
        what = f"{name} n={n}/{A}"
        hs = make()
        nb = [h.nbytes for h in hs]
        failed0 = gpu.alloc_stats().failed
        gpu.alloc_fail_nth(n)
        err = None
        try:
            call(hs)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None, f"{what}: the call succeeded although one of its allocations was to fail"
        assert gpu.alloc_stats().failed - failed0 == 1, what
        assert err.code == gpu.E_NOMEM, f"{what}: {err}"
        assert gpu.load().freddy_gpu_last_error().decode().strip(), what
        assert [h.nbytes for h in hs] == nb, f"{what}: index_bytes moved in a search that failed"
        check(call(hs))                                   # the same call again, nothing armed
        for h in hs:
            h.close()
        assert _live(gpu) == s0, f"{what}: unpin left allocations behind: {_live(gpu)} vs {s0}"
    line = f"alloc-failure sweep {name}: A = {A} allocations (floor {floor}), every one failed once: FREDDY_E_NOMEM, then the expected lists"
    SUMMARY.append(line)
    print(line)


def _lists(exp, what):
    return lambda res: util.assert_same_lists(res[0], res[1], exp(), what)


# =======================================================================================
# pq
# =======================================================================================
# floors (pq.hip): the host-buffer call stages in hio_in + hio_out (:408) = 2; a batch of >= 16 queries over the standard shape builds
# the shadow (pq_view_refresh: viol + six v_* arrays = 7) and its run's workspace (ivf_host.h ivf_run_ensure: 9 at least); a subset
# gathers w_sub_rows / w_sub_packed / w_sub_pos / w_sub_blk (:374) = 4
@pytest.mark.parametrize("form", ["one", "batch", "subset", "dev"])
def test_pq_search(gpu, oracle, tabs, form):
    x = tabs["x"]
    qs = np.ascontiguousarray(x[np.random.default_rng(1).choice(4000, 20, replace=False)])
    sub = np.concatenate([tabs["pq"][1][::5], [10 ** 8]]).astype(np.int32)
    ot = Lazy(lambda: oracle.pq_table(*tabs["pq"]))
    make = lambda: [gpu.PQIndex(*tabs["pq"])]
    if form == "one":
        _sweep(gpu, "pq_search one query", make, lambda h: h[0].search(qs[:1], 5), _lists(Lazy(lambda: oracle.pq_search(ot(), qs[0], 5)[None]), "pq one"), 2)
    elif form == "batch":
        _sweep(gpu, "pq_search batch of 20", make, lambda h: h[0].search(qs, 7), _lists(Lazy(lambda: np.stack([oracle.pq_search(ot(), q, 7) for q in qs])), "pq batch"), 2 + 7 + 9)
    elif form == "subset":
        _sweep(gpu, "pq_search subset", make, lambda h: h[0].search(qs, 5, sentinel=1000.0, subset_ids=sub),
               _lists(Lazy(lambda: oracle.pq_search_in_batch(ot(), qs, 5, sub)), "pq subset"), 2 + 4)
    else:
        import torch
        dq = torch.from_numpy(qs).cuda()
        oi = torch.zeros((20, 7), dtype=torch.int32, device="cuda"); od = torch.zeros((20, 7), dtype=torch.float32, device="cuda")

        def call(h):
            h[0].search_dev(dq.data_ptr(), 20, 7, 100.0, oi.data_ptr(), od.data_ptr())
            torch.cuda.synchronize()
            return oi.cpu().numpy(), od.cpu().numpy()
        _sweep(gpu, "pq_search_dev batch of 20", make, call, _lists(Lazy(lambda: np.stack([oracle.pq_search(ot(), q, 7) for q in qs])), "pq dev"), 7 + 9)


def test_grouping_pq_and_pq_assign(gpu, oracle, tabs):
    """grouping_pq: w_q, w_lut, w_out_ids (pq.hip:489) = 3; pq_assign: w_q, w_lut, w_sub_rows, w_out_ids, w_out_dist, w_found (:539) = 6"""
    x = tabs["x"]
    cb, ids, codes = tabs["pq"]
    gv = np.ascontiguousarray(x[[5, 900, 2000, 5, 3100]])
    ot = Lazy(lambda: oracle.pq_table(*tabs["pq"]))
    make = lambda: [gpu.PQIndex(*tabs["pq"])]

    def check_group(res):
        ei, eg = oracle.grouping_pq(ot(), gv, ids)
        assert np.array_equal(res[0], ei) and np.array_equal(res[1], eg)
    _sweep(gpu, "grouping_pq", make, lambda h: h[0].grouping(gv, None), check_group, 3)
    qs = np.ascontiguousarray(x[[7, 300, 1500, 4100]])
    targets = np.concatenate([ids[::40], [10 ** 8]]).astype(np.int32)
    exp = Lazy(lambda: asm.pq_assign(oracle, cb, ids, codes, qs, targets))

    def check_assign(res):
        eq, es = exp()
        assert np.array_equal(res[0], eq) and np.array_equal(res[1].view(np.uint32), es.view(np.uint32))
    _sweep(gpu, "pq_assign", make, lambda h: h[0].assign(qs, targets), check_assign, 6)


# =======================================================================================
# ivfadc
# =======================================================================================
# floors: one query: hio_out (one.hip ivf_one) + the one-launch buffer w_oneb (one_buffer) = 2; a batch: the staging of either host
# path (pipeline.hip: lane_open's h_in, h_out, d_q, d_ids, d_dist; ivfadc_sync_search's w_q, w_out_ids, w_out_dist) = 3 at least, and
# the run's nine buffers (ivf_run.h ivf_run_ensure) = 12; fused = 0 adds w_resid, w_lut, w_part (ivfadc.hip ivfadc_begin) = 15; k = 600
# adds bigk.h's w_bigsel + w_floor (generic.hip bigk_select_replay) = 14; the device-pointer entry: the nine + w_distT, w_used, w_qn2
# (ivfadc_begin) = 12
@pytest.mark.parametrize("form", ["one", "batch64", "fused0", "k600", "dev"])
def test_ivfadc_search(gpu, oracle, tabs, form):
    x = tabs["x"]
    qs = np.ascontiguousarray(x[np.random.default_rng(2).choice(5900, 64, replace=False)])
    ot = Lazy(lambda: oracle.ivf_table(*tabs["ivf"]))

    def make(opts=()):
        idx = gpu.IVFIndex(*tabs["ivf"])
        for k_, v in opts:
            idx.set_option(k_, v)
        return [idx]
    if form == "one":
        _sweep(gpu, "ivfadc_search one query", make, lambda h: h[0].search(qs[:1], 5, 3), _lists(Lazy(lambda: oracle.ivfadc_search_many(ot(), qs[:1], 5, 3)), "ivf one"), 2)
    elif form == "batch64":
        _sweep(gpu, "ivfadc_search batch of 64 (cell-grouped scan)", lambda: make((("fused", 1),)), lambda h: h[0].search(qs, 5, 3),
               _lists(Lazy(lambda: oracle.ivfadc_search_many(ot(), qs, 5, 3)), "ivf batch"), 12)
    elif form == "fused0":
        _sweep(gpu, "ivfadc_search batch of 64, fused = 0", lambda: make((("fused", 0),)), lambda h: h[0].search(qs, 5, 3),
               _lists(Lazy(lambda: oracle.ivfadc_search_many(ot(), qs, 5, 3)), "ivf fused=0"), 15)
    elif form == "k600":
        _sweep(gpu, "ivfadc_search k = 600 (bigk.h)", make, lambda h: h[0].search(qs[:24], 600, 2),
               _lists(Lazy(lambda: oracle.ivfadc_search_many(ot(), qs[:24], 600, 2)), "ivf k=600"), 14)
    else:
        import torch
        dq = torch.from_numpy(qs).cuda()
        oi = torch.zeros((64, 5), dtype=torch.int32, device="cuda"); od = torch.zeros((64, 5), dtype=torch.float32, device="cuda")
        st = torch.zeros(4, dtype=torch.int32, device="cuda")

        def call(h):
            st.zero_()
            torch.cuda.synchronize()
            h[0].search_dev(dq.data_ptr(), 64, 5, 3, 1000.0, 0, oi.data_ptr(), od.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            assert int(st[0]) == 0, "a query needs a further probing round: the device-pointer entry does not make it"
            return oi.cpu().numpy(), od.cpu().numpy()
        _sweep(gpu, "ivfadc_search_dev batch of 64", make, call, _lists(Lazy(lambda: oracle.ivfadc_search_many(ot(), qs, 5, 3)), "ivf dev"), 12)


# =======================================================================================
# kNN-join
# =======================================================================================
@pytest.mark.parametrize("method", [0, 1, 2])
def test_knn_join(gpu, oracle, tabs, method):
    """join_run.h: JW_QUERIES, JW_SUB, JW_TCELL_OFF, JW_TROW, JW_SCAN, JW_QCELL_OFF, JW_WIN, JW_CELL_CNT, JW_SORTED (:183-187) = 9 and
    the pinned target-list block h_tl (:191) = 10 at least"""
    x = tabs["x"]
    ids = tabs["ivpq"][2]
    rng = np.random.default_rng(3)
    qs = np.ascontiguousarray(x[rng.choice(2900, 12, replace=False)])
    targets = np.concatenate([ids[rng.choice(ids.size, 500, replace=False)], ids[:20], [10 ** 8, -4]]).astype(np.int32)
    exp = Lazy(lambda: oracle.ivpq_search_in(oracle.ivpq_table(*tabs["ivpq"]), qs, 5, targets, 3, 20, method))

    def check(res):
        e, it = exp()
        assert res[2] == it, (res[2], it)
        util.assert_same_lists(res[0], res[1], e, f"knn_join method {method}")
    _sweep(gpu, f"knn_join method {method}", lambda: [gpu.IVPQIndex(*tabs["ivpq"])], lambda h: h[0].knn_join(qs, 5, targets, 3, 20, method), check, 10)


# =======================================================================================
# raw vectors
# =======================================================================================
# floors (exact.hip, exact_host.h): the filter chain: exf_qfrag, exf_sample, exf_cand (exact_filter_search) + viol (ensure_viol) + hio_out (exact_search_rows) = 5;
# all-exact: w_q, w_out_ids, w_out_dist, w_part (exact_search_rows) = 4; analogy: w_rows, w_out_ids, w_out_dist, w_cnt (analogy.hip) = 4;
# exact join: the smaller of its two paths -- vec_subset's w_sub_rows, w_sub_pos, w_resid + the four of the all-exact scan = 7 (the
# filter's path, exact_join_filter, has nine); exact_assign: w_q, w_sub_rows, w_out_ids, w_out_dist (cluster.hip) = 4
@pytest.mark.parametrize("form", ["filter_on", "filter_off", "analogy", "join", "assign"])
def test_exact_calls(gpu, oracle, tabs, form):
    ids, xv = tabs["vec64"]
    rng = np.random.default_rng(4)
    qs = np.ascontiguousarray(xv[rng.choice(8000, 12, replace=False)]); qs[1] = -qs[1]
    sub = np.concatenate([ids[rng.choice(ids.size, 300, replace=False)], [4, 10 ** 8]]).astype(np.int32)

    def make(mode=-1):
        idx = gpu.VectorIndex(ids, xv)
        idx.set_option("exact_filter", mode)
        return [idx]
    full = Lazy(lambda: [oracle.exact_knn(xv, ids, q, 5) for q in qs])
    part = Lazy(lambda: [oracle.exact_knn(xv, ids, q, 5, sub) for q in qs])
    if form == "filter_on":
        _sweep(gpu, "exact_search, filter on", lambda: make(1), lambda h: h[0].search(qs, 5), lambda r: _exact_same(r[0], r[1], full(), 5, "filter on"), 5)
    elif form == "filter_off":
        _sweep(gpu, "exact_search, filter off", lambda: make(0), lambda h: h[0].search(qs, 5), lambda r: _exact_same(r[0], r[1], full(), 5, "filter off"), 4)
    elif form == "analogy":
        triples = ids[rng.integers(0, 8000, size=(6, 3))].copy(); triples[2, 0] = 4
        exp = Lazy(lambda: anm.model(xv, ids, triples, 4, "3cosadd"))

        def check(r):
            ei, es = exp()
            assert np.array_equal(r[0], ei) and np.array_equal(r[1].view(np.uint64), es.view(np.uint64))
        _sweep(gpu, "exact_analogy 3cosadd", make, lambda h: h[0].analogy(triples, k=4, method="3cosadd"), check, 4)
    elif form == "join":
        _sweep(gpu, "exact_join", make, lambda h: h[0].join(qs, 5, sub), lambda r: _exact_same(r[0], r[1], part(), 5, "exact join"), 7)
    else:
        exp = Lazy(lambda: asm.exact_assign(ids, xv, qs, sub))

        def check(r):
            eq, es = exp()
            assert np.array_equal(r[0], eq) and np.array_equal(r[1].view(np.uint32), es.view(np.uint32))
        _sweep(gpu, "exact_assign", make, lambda h: h[0].assign(qs, sub), check, 4)


# =======================================================================================
# two handles: post verification and the approximate analogies (rerank.hip rerank_block: pv_io + pv_q = 2, and the search's own buffers)
# =======================================================================================
@pytest.mark.parametrize("ann", ["ivf", "pq"])
@pytest.mark.parametrize("what", ["search_pv", "analogy"])
def test_two_handle_calls(gpu, oracle, tabs, ann, what):
    x = tabs["x"]
    vid, vx = tabs["vec300"]
    rng = np.random.default_rng(5)
    qs = np.ascontiguousarray(x[rng.choice(1900, 10, replace=False)])
    triples = vid[rng.integers(0, 1900, size=(6, 3))].astype(np.int32)
    make = lambda: [gpu.IVFIndex(*tabs["ivf"]) if ann == "ivf" else gpu.PQIndex(*tabs["pq"]), gpu.VectorIndex(vid, vx)]
    table = Lazy(lambda: oracle.ivf_table(*tabs["ivf"]) if ann == "ivf" else oracle.pq_table(*tabs["pq"]))
    k, pvf, n_cand, W = 3, 8, 23, 3
    if what == "search_pv":
        lists = Lazy(lambda: pm.ivf_lists(oracle, table(), qs, k * pvf, W) if ann == "ivf" else pm.pq_lists(oracle, table(), qs, k * pvf))
        exp = Lazy(lambda: pm.expected(oracle, lists(), vx, vid, qs, k)[0])
        call = (lambda h: h[0].search_pv(h[1], qs, k, pvf, W)) if ann == "ivf" else (lambda h: h[0].search_pv(h[1], qs, k, pvf))
        _sweep(gpu, f"{ann}_search_pv", make, call, lambda r: pm.same(r[0], r[1], exp(), k, f"{ann} pv"), 2 + 2)
    else:
        exp = Lazy(lambda: (aam.ivf_expected(oracle, table(), vx, vid, triples, k, n_cand, W) if ann == "ivf" else aam.pq_expected(oracle, table(), vx, vid, triples, k, n_cand))[0])
        call = (lambda h: h[0].analogy(h[1], triples, k, n_cand, W)) if ann == "ivf" else (lambda h: h[0].analogy(h[1], triples, k, n_cand))
        _sweep(gpu, f"{ann}_analogy", make, call, lambda r: pm.same(r[0], r[1], exp(), k, f"{ann} analogy"), 2 + 2)


# =======================================================================================
# the stand-alone calls (build.hip; core.hip host_alloc)
# =======================================================================================
def test_encode_kmeans_insert_quantize_host_alloc(gpu, oracle, tabs):
    """encode: d_cbT, d_vec, d_codes (build.hip:50-52) = 3, with a coarse quantizer + d_cT, d_coarse, d_res, d_cell = 7; kmeans: d_vec,
    d_cent, d_centT, d_assign = 4; insert_quantize with the PQ codebook and the residual codebook: two encodes, each + d_far = 4 + 8;
    host_alloc: the one pinned block"""
    x = tabs["x"]
    cb = tabs["pq"][0]
    coarse, rcb = tabs["ivf"][0], tabs["ivf"][1]
    v = np.ascontiguousarray(x[100:170])
    none = lambda: []
    exp_codes = Lazy(lambda: oracle.encode_pq(cb, v))
    _sweep(gpu, "encode", none, lambda h: gpu.encode(cb, v), lambda r: np.testing.assert_array_equal(r[1], exp_codes()), 3)
    exp_cell = Lazy(lambda: oracle.assign_coarse(coarse, v))

    def check_res(r):
        cell = exp_cell()
        assert np.array_equal(r[0], cell)
        assert np.array_equal(r[1], oracle.encode_pq(rcb, np.stack([oracle.vec_minus(a, coarse[c]) for a, c in zip(v, cell)])))
    _sweep(gpu, "encode with a coarse quantizer", none, lambda h: gpu.encode(rcb, v, coarse=coarse), check_res, 7)
    init = np.arange(0, 70, 10, dtype=np.int32)
    exp_km = Lazy(lambda: oracle.kmeans(v, 7, 3, init))

    def check_km(r):
        oc, oa = exp_km()
        assert np.array_equal(r[1], oa) and np.array_equal(r[0].view(np.uint32), oc.view(np.uint32))
    _sweep(gpu, "kmeans", none, lambda h: gpu.kmeans(v, 7, 3, init), check_km, 4)

    def check_iq(r):
        assert np.array_equal(r["pq_codes"], exp_codes())
        assert np.array_equal(r["coarse_id"], exp_cell())
    _sweep(gpu, "insert_quantize", none, lambda h: gpu.insert_quantize(v, pq_codebook=cb, residual_codebook=rcb, coarse=coarse), check_iq, 4 + 8)

    def host_alloc(h):
        p = C.c_void_p()
        rc = gpu.load().freddy_gpu_host_alloc(C.byref(p), 4096)
        if rc:
            assert p.value is None, "*out is not NULL after a failed host_alloc"
            gpu._check(rc)
        assert p.value
        gpu._check(gpu.load().freddy_gpu_host_free(p))
        return True
    _sweep(gpu, "host_alloc", none, host_alloc, lambda r: None, 1)


# =======================================================================================
# the steady state allocates nothing; one failure that is the runtime's own
# =======================================================================================
def test_steady_state_allocates_nothing(gpu, oracle, tabs):
    """bench.py's timed region: ivfadc_search_dev on four streams with scan_share = 4; and the host-buffer ivfadc_search at 1024
    queries.  After the warm-up, 20 identical calls of each move the seam's call counter by ZERO: every buffer is there, nothing in
    the timed region reaches an allocation -- and it stays that way."""
    import torch
    x = tabs["x"]
    idx = gpu.IVFIndex(*tabs["ivf"])
    idx.set_option("scan_share", 4)
    Q = 256
    rng = np.random.default_rng(6)
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = []
    for s in range(4):
        dq = torch.from_numpy(np.ascontiguousarray(x[rng.choice(5900, Q, replace=False)])).cuda()
        bufs.append((dq, torch.zeros((Q, 5), dtype=torch.int32, device="cuda"), torch.zeros((Q, 5), dtype=torch.float32, device="cuda"),
                     torch.zeros(4, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()

    def round_dev():
        for s, (dq, oi, od, st) in zip(streams, bufs):
            idx.search_dev(dq.data_ptr(), Q, 5, 3, 1000.0, 0, oi.data_ptr(), od.data_ptr(), st.data_ptr(), s.cuda_stream)
    for _ in range(2):
        round_dev()
    torch.cuda.synchronize()
    c0 = gpu.alloc_stats().calls
    for _ in range(20):
        round_dev()
    torch.cuda.synchronize()
    assert gpu.alloc_stats().calls == c0, f"20 rounds of four ivfadc_search_dev calls allocated {gpu.alloc_stats().calls - c0} times"
    ot = oracle.ivf_table(*tabs["ivf"])
    dq, oi, od, st = bufs[0]
    util.assert_same_lists(oi.cpu().numpy(), od.cpu().numpy(), oracle.ivfadc_search_many(ot, dq.cpu().numpy(), 5, 3, n_threads=8), "steady state, stream 0")
    qs = np.ascontiguousarray(x[rng.choice(5900, 1024, replace=False)])
    for _ in range(2):
        got = idx.search(qs, 5, 3)
    c0 = gpu.alloc_stats().calls
    for _ in range(20):
        got = idx.search(qs, 5, 3)
    assert gpu.alloc_stats().calls == c0, f"20 host-buffer searches of 1024 queries allocated {gpu.alloc_stats().calls - c0} times"
    util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(ot, qs, 5, 3, n_threads=8), "steady state, host buffer")
    idx.close()


def test_a_failure_of_the_runtime_itself_leaves_the_next_search_healthy(gpu, oracle, tabs):
    """The second mode of the seam: the armed allocation -- the first DevBuf::ensure of a cold workspace -- is forwarded to hipMalloc
    with a request for 2^60 bytes, so the runtime's own error state is that of a real failure.  The call reports FREDDY_E_NOMEM; the
    VERY NEXT search on the handle returns FREDDY_OK and the oracle's lists: the wrapper has cleared the runtime's last-error word,
    which the hipGetLastError() behind every launch would otherwise report as that launch's."""
    import torch
    x = tabs["x"]
    qs = np.ascontiguousarray(x[np.random.default_rng(7).choice(5900, 64, replace=False)])
    idx = gpu.IVFIndex(*tabs["ivf"])
    dq = torch.from_numpy(qs).cuda()
    oi = torch.zeros((64, 5), dtype=torch.int32, device="cuda"); od = torch.zeros((64, 5), dtype=torch.float32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    failed0 = gpu.alloc_stats().failed
    gpu.alloc_fail_nth(1, real=True)
    try:
        with pytest.raises(gpu.FreddyGpuError) as e:
            idx.search_dev(dq.data_ptr(), 64, 5, 3, 1000.0, 0, oi.data_ptr(), od.data_ptr(), st.data_ptr())
    finally:
        gpu.alloc_fail_nth(0)
    assert e.value.code == gpu.E_NOMEM, str(e.value)
    assert gpu.alloc_stats().failed - failed0 == 1
    idx.search_dev(dq.data_ptr(), 64, 5, 3, 1000.0, 0, oi.data_ptr(), od.data_ptr(), st.data_ptr())   # raises unless FREDDY_OK
    torch.cuda.synchronize()
    exp = oracle.ivfadc_search_many(oracle.ivf_table(*tabs["ivf"]), qs, 5, 3)
    util.assert_same_lists(oi.cpu().numpy(), od.cpu().numpy(), exp, "the search after the runtime's own failure")
    got = idx.search(qs, 5, 3)
    util.assert_same_lists(got[0], got[1], exp, "the host-buffer search after it")
    idx.close()
