"""-m gpu: the contract of the device-pointer searches (include/freddy_gpu.h: freddy_gpu_ivfadc_search_dev, freddy_gpu_pq_search_dev).

The status word is the only evidence a caller of the *_dev entry points has that its buffers hold complete lists, and the
host-buffer calls never read it (they read the straggler count beside it).  Every case here runs a batch whose set of unfinished
queries is known from the capped CPU oracle (tests/dev_contract_inputs.py, proven on the CPU by test_dev_contract_inputs_cpu.py) and
asserts, in this order: the intended kernels ran; every list is the oracle's ROUND-ONE list (for a finished query also its
final list); the unfinished queries re-run through the host-buffer call give the final lists; no bracket was violated; and, last,
status != 0 <=> the oracle says some query of the batch is unfinished.  (Last, so that a library that never wrote the word fails
the mixed and the all batches on that line alone.)  Ids, ranks and distance bits throughout."""
import ctypes as C

import numpy as np
import pytest

import dev_contract_inputs as dci
import util

pytestmark = pytest.mark.gpu

E_ARG, E_KIND, E_LIMIT = -1, -4, -5   # include/freddy_gpu.h


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def pins(gpu):
    """One pinned handle per thinned table, shared by the cases of this module."""
    held = {}

    def get(key):
        if key not in held:
            c = dci.case(*key)
            held[key] = gpu.IVFIndex(c["coarse"], c["codebook"], c["list_off"], c["ids"], c["codes"])
        return held[key]
    yield get
    for idx in held.values():
        idx.close()


DEFAULTS = {"fused": -1, "fused_kernel": 5, "scan_share": 0, "lut_budget_mb": 8192}


def _options(idx, opts):
    for name, value in {**DEFAULTS, **opts}.items():
        idx.set_option(name, value)


def _dev(qs, k, fill_id=-7):
    """Device buffers of one call: queries, ids and distances preset to a pattern no search writes, a zeroed status word."""
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.array(qs, np.float32)).to(dev)     # (a copy: the shared inputs are read-only)
    oi = torch.full((qs.shape[0], k), fill_id, dtype=torch.int32, device=dev)
    od = torch.full((qs.shape[0], k), -3.0, dtype=torch.float32, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    return dq, oi, od, st


def _search_dev(idx, qs, k, W, sentinel, rule, stream, with_status=True):
    """One profiled freddy_gpu_ivfadc_search_dev call on `stream` (None: the library's own), the word zeroed first on the same
    stream.  -> (ids, dist, status word, {kernel: launches})"""
    import torch
    dq, oi, od, st = _dev(qs, k)
    idx.profile_enable(True)
    if stream is None:
        idx.search_dev(dq.data_ptr(), qs.shape[0], k, W, sentinel, rule, oi.data_ptr(), od.data_ptr(), st.data_ptr() if with_status else 0, None)
    else:
        with torch.cuda.stream(stream):
            st.zero_()
            idx.search_dev(dq.data_ptr(), qs.shape[0], k, W, sentinel, rule, oi.data_ptr(), od.data_ptr(),
                           st.data_ptr() if with_status else 0, stream.cuda_stream)
    torch.cuda.synchronize()
    prof = {name: n for name, (n, _) in idx.profile_read().items()}
    idx.profile_enable(False)
    return oi.cpu().numpy(), od.cpu().numpy(), int(st[0].item()), prof


def _assert_round_one(gi, gd, exp, what):
    util.assert_same_lists(gi, gd, exp["round_one"], what + ": round-one lists")
    fin = ~exp["unfinished"]
    util.assert_same_lists(gi[fin], gd[fin], exp["final"][fin], what + ": final lists of the finished queries")


def _assert_protocol(idx, qs, k, W, sentinel, rule, exp, what):
    """What the header prescribes for the unfinished queries: the host-buffer call gives their complete lists."""
    unf = exp["unfinished"]
    if unf.any():
        hi, hd = idx.search(qs[unf], k, W, sentinel=sentinel, found_rule=rule)
        util.assert_same_lists(hi, hd, exp["final"][unf], what + ": unfinished queries through the host-buffer call")


# path id -> (option settings, kernels that must run, kernels that must not)
PATHS = {
    "filter": ({"fused": 1}, {"ivf_filter", "merge_refine"}, {"merge_surv", "merge_replay", "adc_scan"}),
    "inflight": ({"fused": 1, "scan_share": 4}, {"ivf_filter", "merge_refine"}, {"merge_surv", "merge_replay", "adc_scan"}),
    "exact": ({"fused": 1, "fused_kernel": 3}, {"ivf_exact_scan", "merge_surv"}, {"ivf_filter", "merge_refine", "merge_replay"}),
    "multi": ({"fused": 1}, {"ivf_multi_scan", "merge_surv"}, {"ivf_filter", "merge_refine", "merge_replay"}),
    "generic": ({"fused": 0}, {"lut_build", "adc_scan", "merge_replay"}, {"ivf_filter", "merge_surv", "merge_refine", "bigk_replay"}),
    "ties": ({"fused": 0}, {"lut_build", "adc_scan", "merge_replay"}, {"ivf_filter", "merge_surv", "merge_refine", "bigk_replay"}),
    "wide": ({"fused": 1}, {"lut_build", "adc_scan", "merge_replay"}, {"ivf_filter", "merge_surv", "merge_refine", "bigk_replay"}),
    "bigk": ({"fused": 1}, {"adc_scan", "merge_select", "bigk_replay"}, {"ivf_filter", "merge_surv", "merge_refine", "merge_replay"}),
}
# (path, table) -- dci.CASES names the W each table runs with
RUNS = [("filter", ("300", 256, 5, False)), ("filter", ("300", 256, 32, False)), ("filter", ("300", 1024, 5, False)), ("filter", ("300", 1024, 32, False)),
        ("inflight", ("300", 256, 32, False)), ("inflight", ("300", 1024, 5, False)),
        ("exact", ("300", 256, 5, False)), ("exact", ("300", 1024, 32, False)),
        ("multi", ("64", 16, 5, False)),
        ("generic", ("300", 256, 5, False)), ("ties", ("300", 256, 5, True)),
        ("wide", ("300", 256, 40, False)), ("bigk", ("300", 256, 600, False))]
RUN_IDS = [f"{p}-K{c[1]}-k{c[2]}" for p, c in RUNS]


@pytest.mark.parametrize("batch", dci.BATCHES)
@pytest.mark.parametrize("path,key", RUNS, ids=RUN_IDS)
def test_status_word_and_round_one_lists(gpu, pins, path, key, batch):
    import torch
    shape, K, k, ties = key
    opts, must, must_not = PATHS[path]
    c = dci.case(*key)
    idx = pins(key)
    _options(idx, opts)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    verdicts = []
    for W in dci.CASES[key]:
        qs, _ = dci.batches(shape, K, k, ties, W)[batch]
        for rule in dci.RULES[W]:
            exp = dci.expected(shape, K, k, ties, W, rule, batch)
            sent = dci.sentinel_of(c, rule)
            what = f"{path} K={K} k={k} W={W} rule={rule} {batch}"
            gi, gd, status, prof = _search_dev(idx, qs, k, W, sent, rule, stream)
            assert must <= set(prof) and not must_not & set(prof), (what, sorted(prof))
            _assert_round_one(gi, gd, exp, what)
            _assert_protocol(idx, qs, k, W, sent, rule, exp, what)
            verdicts.append((what, status, bool(exp["unfinished"].any())))
    assert idx.bound_violations() == 0
    _options(idx, {})
    for what, status, some_unfinished in verdicts:
        assert (status != 0) == some_unfinished, f"{what}: status word {status}, the oracle says unfinished = {some_unfinished}"


@pytest.mark.parametrize("path,key", [r for r in RUNS if r[0] in ("filter", "exact", "multi", "generic", "ties") and r[1][2] == 5], ids=lambda v: v if isinstance(v, str) else f"K{v[1]}")
def test_one_unfinished_query_among_finished_ones(gpu, pins, path, key):
    """In an `all` batch every query sets the word, so a write missing from ONE place of a kernel hides behind the others:
    merge_replay_kernel sets it on its no-tie fast path (the empty cell, the cells of one row) and on its replay path (the cell of
    k - 1 rows of the `ties` table, whose rows pair up at equal distances; test_dev_contract_inputs_cpu.py).  Here 63 finished
    queries and ONE designed query per call, for every designed query that is unfinished with one probe."""
    import torch
    shape, K, k, ties = key
    opts, must, must_not = PATHS[path]
    c = dci.case(*key)
    idx = pins(key)
    _options(idx, opts)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    none = dci.batches(shape, K, k, ties, 1)["none"][0][:63]
    verdicts = []
    for name in ["E", "O", "M"] + [f"G{j}" for j in range(8)]:
        qs = np.concatenate([none[:17], c["designed"][name][None, :], none[17:]]).astype(np.float32)
        for rule in (0, 1):
            one, found, _ = dci.search(c, qs, k, 1, rule, 1)
            assert np.array_equal(np.nonzero(found < k)[0], [17]), "input"
            gi, gd, status, prof = _search_dev(idx, qs, k, 1, c["sentinel"], rule, stream)
            assert must <= set(prof) and not must_not & set(prof), (path, name, sorted(prof))
            util.assert_same_lists(gi, gd, one, f"{path} one unfinished query ({name}) rule={rule}")
            verdicts.append((name, rule, status))
    assert idx.bound_violations() == 0
    _options(idx, {})
    for name, rule, status in verdicts:
        assert status != 0, f"{path}: the only unfinished query ({name}, rule {rule}) left the word at 0"


def _reuse(gpu, pins, stream):
    """An all-unfinished batch, the word zeroed, then a none-unfinished batch of another Q and k on the same stream: what the
    first call left in found, next_active and n_next must not reach the second."""
    key = ("300", 256, 32, False)
    c = dci.case(*key)
    idx = pins(key)
    _options(idx, {"fused": 1})
    qa, _ = dci.batches(*key, 1)["all"]
    qn = dci.batches(*key, 1)["none"][0][:100]
    for rule in (0, 1):
        ea = dci.expected(*key, 1, rule, "all")
        one, found, _ = dci.search(c, qn, 5, 1, rule, 1)
        assert (found >= 5).all(), "input: a query of the second batch is unfinished at k = 5"
        gi, gd, status, _ = _search_dev(idx, qa, 32, 1, c["sentinel"], rule, stream)
        _assert_round_one(gi, gd, ea, f"reuse rule={rule}: first call")
        assert status != 0, f"reuse rule={rule}: the all-unfinished batch left the word at 0"
        gi, gd, status, _ = _search_dev(idx, qn, 5, 1, c["sentinel"], rule, stream)
        util.assert_same_lists(gi, gd, one, f"reuse rule={rule}: second call")
        util.assert_same_lists(gi, gd, dci.search(c, qn, 5, 1, rule, 0)[0], f"reuse rule={rule}: second call, final lists")
        assert status == 0, f"reuse rule={rule}: the word is {status} after a batch without unfinished queries"
    return idx, c, qn


def test_stream_reuse(gpu, pins):
    import torch
    idx, _, _ = _reuse(gpu, pins, torch.cuda.Stream(torch.device("cuda", 0)))
    assert idx.bound_violations() == 0
    _options(idx, {})


def test_default_stream_then_host_buffer_call(gpu, pins):
    """hip_stream = NULL: the library's own stream and workspace, which the host-buffer call on the same handle uses next."""
    idx, c, qn = _reuse(gpu, pins, None)
    hi, hd = idx.search(qn, 5, 1, sentinel=c["sentinel"], found_rule=0)
    util.assert_same_lists(hi, hd, dci.search(c, qn, 5, 1, 0, 0)[0], "host-buffer call after the NULL-stream calls")
    qm, _ = dci.batches("300", 256, 32, False, 1)["mixed"]
    hi, hd = idx.search(qm, 32, 1, sentinel=c["sentinel"], found_rule=1)
    util.assert_same_lists(hi, hd, dci.expected("300", 256, 32, False, 1, 1, "mixed")["final"], "host-buffer call, mixed batch")
    assert idx.bound_violations() == 0
    _options(idx, {})


def _max_queries_per_chunk(mb, m, K, W, upi, C_):
    """csrc/ivfadc.hip max_queries_per_chunk for a 300-d / m = 12 table and 2k <= 64: the LUTs of a query's W items or their
    survivor regions (8 waves x 8 x 64 keys of 8 bytes per 4096-row unit), whichever is larger, within lut_budget_mb."""
    per_query = max(4 * m * K * W, 8 * W * upi * 8 * 8 * 64)
    n = min((mb << 20) // per_query, (256 << 20) // (4 * C_))
    return max(1, min(n, 1 << 20))


@pytest.mark.parametrize("where", ["first", "last"])
def test_chunked_call_shares_the_word(gpu, pins, where):
    """lut_budget_mb cuts Q = 300 into chunks; the unfinished queries all sit in the first or in the last one.  The word is set
    either way (the chunks share it and the library never clears it) and every chunk's lists land at its offset."""
    import torch
    key, W, rule = ("300", 256, 5, False), 1, 0
    c = dci.case(*key)
    idx = pins(key)
    qs, _ = dci.batches(*key, W)["mixed"]
    exp = dci.expected(*key, W, rule, "mixed")
    n_unf = int(exp["unfinished"].sum())
    assert np.diff(c["list_off"]).max() <= 4096   # (one survivor unit per item)
    fits = [mb for mb in range(1, 65) for per in [_max_queries_per_chunk(mb, 12, 256, W, 1, 64)]
            if -(-300 // per) >= 3 and min(per, 300 - (-(-300 // per) - 1) * per) >= n_unf]
    assert fits, "no lut_budget_mb gives three chunks whose first and last hold the unfinished queries"
    mb = max(fits)
    per = _max_queries_per_chunk(mb, 12, 256, W, 1, 64)
    chunks = -(-300 // per)
    order = np.argsort(~exp["unfinished"] if where == "first" else exp["unfinished"], kind="stable")
    lo, hi = (0, per) if where == "first" else ((chunks - 1) * per, 300)
    at = np.nonzero(exp["unfinished"][order])[0]
    assert at.min() >= lo and at.max() < hi, "input: an unfinished query lies outside the intended chunk"
    e = {name: exp[name][order] for name in ("round_one", "unfinished", "final")}
    _options(idx, {"fused": 1, "lut_budget_mb": mb})
    gi, gd, status, prof = _search_dev(idx, qs[order], 5, W, c["sentinel"], rule, torch.cuda.Stream(torch.device("cuda", 0)))
    _options(idx, {})
    assert prof.get("merge_refine") == chunks and prof.get("ivf_filter") == chunks, (chunks, prof)
    _assert_round_one(gi, gd, e, f"chunked, unfinished in the {where} of {chunks} chunks")
    assert idx.bound_violations() == 0
    assert status != 0, f"unfinished queries in the {where} of {chunks} chunks left the word at 0"


def test_null_status_pointer(gpu, pins):
    """d_status == NULL is allowed: the same lists as with a word."""
    import torch
    key = ("300", 1024, 5, False)
    c = dci.case(*key)
    idx = pins(key)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for opts in ({"fused": 1}, {"fused": 0}, {"fused": 1, "fused_kernel": 3}):
        _options(idx, opts)
        for W, rule in ((4, 0), (1, 1)):
            qs, _ = dci.batches(*key, W)["mixed"]
            exp = dci.expected(*key, W, rule, "mixed")
            wi, wd, status, _ = _search_dev(idx, qs, 5, W, c["sentinel"], rule, stream)
            ni, nd, untouched, _ = _search_dev(idx, qs, 5, W, c["sentinel"], rule, stream, with_status=False)
            _assert_round_one(ni, nd, exp, f"NULL status {opts} W={W} rule={rule}")
            assert np.array_equal(wi, ni) and np.array_equal(wd.view(np.uint32), nd.view(np.uint32))
            assert status != 0 and untouched == 0
    _options(idx, {})


@pytest.mark.parametrize("fused", [-1, 1, 0])
def test_all_cells_probed_and_fewer_than_k_rows(gpu, fused):
    """W >= C on a table of fewer than k rows: by the definition (found < k after round one) every query is unfinished although
    no further round can add anything -- the word is set, every row is listed, the other slots hold (-1, sentinel)."""
    import torch
    c = dci.case("300", 256, 5, False)
    cells = [c["cells"]["O"], c["cells"]["M"]] + c["G"]
    C_ = c["coarse"].shape[0]
    cell_of = np.repeat(np.arange(C_), np.diff(c["list_off"]))
    keep = np.isin(cell_of, cells)
    off = np.concatenate([[0], np.cumsum(np.bincount(cell_of[keep], minlength=C_))]).astype(np.int32)
    ids, codes = c["ids"][keep], c["codes"][keep]
    rows, k = int(keep.sum()), 10
    assert rows == 9 < k
    o = dci.oracle()
    ot = o.ivf_table(c["coarse"], c["codebook"], off, ids, codes)
    idx = gpu.IVFIndex(c["coarse"], c["codebook"], off, ids, codes)
    idx.set_option("fused", fused)
    qs = np.concatenate([np.stack(list(c["designed"].values())), c["corpus"][:27]])
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for W in (C_, C_ + 36):
        for rule in (0, 1):
            one, found, _ = o.ivfadc_search_many(ot, qs, k, W, sentinel=1000.0, found_rule=rule, max_rounds=1)
            final = o.ivfadc_search_many(ot, qs, k, W, sentinel=1000.0, found_rule=rule)
            assert (found == rows).all() and np.array_equal(one, final)
            gi, gd, status, _ = _search_dev(idx, qs, k, W, 1000.0, rule, stream)
            util.assert_same_lists(gi, gd, one, f"W={W} >= C rule={rule} fused={fused}")
            assert (np.sort(gi[:, :rows], axis=1) == np.sort(ids)).all(), "not every row is listed"
            assert (gi[:, rows:] == -1).all() and (gd[:, rows:] == np.float32(1000.0)).all()
            hi, hd = idx.search(qs, k, W, sentinel=1000.0, found_rule=rule)
            util.assert_same_lists(hi, hd, final, f"W={W} >= C rule={rule} fused={fused}: host-buffer call")
            assert status != 0, f"W={W} >= C rule={rule} fused={fused}: found = {rows} < k = {k} and the word is 0"
    idx.close()


# ---- refusals: nothing is enqueued ------------------------------------------------------------------------------------------
def _quiet(gpu, idx, call, code, what):
    """`call` returns `code`, allocates nothing and launches nothing on `idx`."""
    calls = gpu.alloc_stats().calls
    idx.profile_enable(True)
    rc = call()
    prof = idx.profile_read()
    idx.profile_enable(False)
    assert rc == code, f"{what}: returned {rc} ({gpu.load().freddy_gpu_last_error().decode()}), expected {code}"
    assert gpu.alloc_stats().calls == calls, f"{what}: an allocation was made"
    assert sum(n for n, _ in prof.values()) == 0, f"{what}: launched {prof}"


def test_refusals_enqueue_nothing(gpu, pins):
    import torch
    lib = gpu.load()
    key = ("300", 256, 5, False)
    c = dci.case(*key)
    ivf = pins(key)
    t = util.pq_tables(N=20000, K=256)
    pq = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    x = util.corpus(20000)[:64].numpy().astype(np.float32)
    vec = gpu.VectorIndex(np.arange(1, 65, dtype=np.int32), x)
    qs = dci.batches(*key, 1)["none"][0][:8]
    dq, oi, od, st = _dev(qs, 5)
    Q, q, i, d, s = 8, dq.data_ptr(), oi.data_ptr(), od.data_ptr(), st.data_ptr()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    hs = stream.cuda_stream

    def ivf_call(h=None, q=q, Q=Q, k=5, W=3, rule=0, i=i, d=d):
        return lambda: lib.freddy_gpu_ivfadc_search_dev(ivf.h if h is None else h, q, Q, k, W, C.c_float(1000.0), rule, i, d, s, hs)

    def pq_call(h=None, q=q, Q=Q, k=5, i=i, d=d):
        return lambda: lib.freddy_gpu_pq_search_dev(pq.h if h is None else h, q, Q, k, C.c_float(100.0), i, d, hs)

    for what, call, code in (("k = 0", ivf_call(k=0), E_ARG), ("k = -3", ivf_call(k=-3), E_ARG), ("k = 4097", ivf_call(k=4097), E_LIMIT),
                             ("W = 0", ivf_call(W=0), E_ARG), ("W = -1", ivf_call(W=-1), E_ARG), ("found rule 3", ivf_call(rule=3), E_ARG),
                             ("found rule -1", ivf_call(rule=-1), E_ARG), ("rule 2 with W = 2", ivf_call(rule=2, W=2), E_ARG),
                             ("NULL queries", ivf_call(q=None), E_ARG), ("NULL ids", ivf_call(i=None), E_ARG), ("NULL distances", ivf_call(d=None), E_ARG),
                             ("NULL handle", lambda: lib.freddy_gpu_ivfadc_search_dev(None, q, Q, 5, 3, C.c_float(1000.0), 0, i, d, s, hs), E_ARG),
                             ("Q = -1", ivf_call(Q=-1), E_ARG),
                             ("a pq handle", ivf_call(h=pq.h), E_KIND), ("a vector handle", ivf_call(h=vec.h), E_KIND)):
        _quiet(gpu, ivf, call, code, "ivfadc_search_dev, " + what)
    for what, call, code in (("k = 0", pq_call(k=0), E_ARG), ("k = 4097", pq_call(k=4097), E_LIMIT), ("Q = -1", pq_call(Q=-1), E_ARG),
                             ("NULL queries", pq_call(q=None), E_ARG), ("NULL ids", pq_call(i=None), E_ARG), ("NULL distances", pq_call(d=None), E_ARG),
                             ("NULL handle", lambda: lib.freddy_gpu_pq_search_dev(None, q, Q, 5, C.c_float(100.0), i, d, hs), E_ARG),
                             ("an ivf handle", pq_call(h=ivf.h), E_KIND), ("a vector handle", pq_call(h=vec.h), E_KIND)):
        _quiet(gpu, pq, call, code, "pq_search_dev, " + what)
    # Q = 0 succeeds (NULL buffers included), writes nothing and leaves the word alone
    for what, idx, call in (("ivfadc_search_dev", ivf, ivf_call(Q=0)), ("ivfadc_search_dev, NULL buffers", ivf, ivf_call(Q=0, q=None, i=None, d=None)),
                            ("pq_search_dev", pq, pq_call(Q=0)), ("pq_search_dev, NULL buffers", pq, pq_call(Q=0, q=None, i=None, d=None))):
        _quiet(gpu, idx, call, 0, what + ", Q = 0")
    torch.cuda.synchronize()
    assert (oi == -7).all().item() and (od == -3.0).all().item() and int(st[0].item()) == 0, "a refused or empty call wrote to the caller's buffers"
    pq.close()
    vec.close()


def test_more_than_512_probes_is_refused(gpu):
    """W is cut to the number of cells first, so the limit of 512 probes per round shows on a table of more cells only: C = 520
    cells of two rows, W = 513."""
    import torch
    t = util.shape_ivf_tables(64, 8, 16, 16, 8000)
    rng = np.random.default_rng(9)
    C_ = 520
    coarse = rng.standard_normal((C_, 64)).astype(np.float32)
    idx = gpu.IVFIndex(coarse, t["codebook"], (np.arange(C_ + 1) * 2).astype(np.int32), np.arange(1, 2 * C_ + 1, dtype=np.int32),
                       rng.integers(0, 16, size=(2 * C_, 8)).astype(np.int16))
    dq, oi, od, st = _dev(coarse[:8], 5)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    lib = gpu.load()
    for fused in (-1, 1, 0):
        idx.set_option("fused", fused)
        _quiet(gpu, idx, lambda: lib.freddy_gpu_ivfadc_search_dev(idx.h, dq.data_ptr(), 8, 5, 513, C.c_float(1000.0), 0, oi.data_ptr(), od.data_ptr(),
                                                                   st.data_ptr(), stream.cuda_stream), E_LIMIT, f"W = 513, fused = {fused}")
        assert "W=513" in lib.freddy_gpu_last_error().decode()
    torch.cuda.synchronize()
    assert (oi == -7).all().item() and int(st[0].item()) == 0
    idx.close()


# ---- freddy_gpu_pq_search_dev -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pq_case():
    """K -> (table, 300 queries, the sentinel inside the data): a flat PQ table is an IVF table of ONE cell with a zero centroid
    (the residual q - 0 is q, bit for bit), which gives the oracle's pq_search a sentinel argument: with 100.0 the two agree."""
    held = {}

    def get(K):
        if K not in held:
            o = dci.oracle()
            t = util.pq_tables(N=20000, K=K)
            _, qs = util.queries_from_corpus(20000, 300, seed=41)
            ot = o.ivf_table(np.zeros((1, 300), np.float32), t["codebook"], np.array([0, 20000], np.int32), t["ids"], t["codes"])
            pt = o.pq_table(t["codebook"], t["ids"], t["codes"])
            for q in qs[:3]:
                assert np.array_equal(o.pq_search(pt, q, 33), o.ivfadc_search(ot, q, 33, 1, sentinel=100.0, found_rule=0))
            inside = float(np.median(o.ivfadc_search_many(ot, qs, 7, 1, sentinel=100.0, n_threads=8)["dist"][:, 3]))
            held[K] = (t, qs, ot, inside)
        return held[K]
    return get


@pytest.mark.parametrize("k", [1, 7, 33, 600])
@pytest.mark.parametrize("K", [256, 1024])
def test_pq_search_dev(gpu, pq_case, K, k):
    """Q = 1, 15, 16 (the cell-grouped scan starts at 16 queries) and 300; sentinel 100.0 and one inside the data (about half the
    queries have fewer than four rows below it); an explicit stream and the NULL stream; lists preset to a pattern."""
    import torch
    t, qs, ot, inside = pq_case(K)
    o = dci.oracle()
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for sent in (100.0, inside):
        exp = o.ivfadc_search_many(ot, qs, k, 1, sentinel=sent, found_rule=0, n_threads=8)
        if sent == inside:
            n_real = (exp["id"] >= 0).sum(1)
            assert (n_real < min(k, 4)).any() and (n_real > 0).any(), "input: the sentinel is not inside the data"
        for Q in (1, 15, 16, 300):
            for s in (stream, None):
                dq, oi, od, _ = _dev(qs[:Q], k)
                idx.profile_enable(True)
                idx.search_dev(dq.data_ptr(), Q, k, sent, oi.data_ptr(), od.data_ptr(), None if s is None else s.cuda_stream)
                torch.cuda.synchronize()
                names = set(idx.profile_read())
                idx.profile_enable(False)
                what = f"pq_search_dev K={K} k={k} Q={Q} sentinel={sent!r} stream={'own' if s is None else 'caller'}"
                util.assert_same_lists(oi.cpu().numpy(), od.cpu().numpy(), exp[:Q], what)
                if Q >= 16 and 2 * k <= 64:
                    assert "ivf_filter" in names and "merge_refine" in names, (what, sorted(names))
                else:
                    assert "adc_scan" in names and "ivf_filter" not in names and ("bigk_replay" in names) == (k == 600), (what, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()
