"""-m gpu: a search call gives the same lists however option lut_budget_mb cuts its queries into chunks (include/freddy_gpu.h).

The chunk loop (for_chunks, csrc/ivf_run.h) runs in freddy_gpu_ivfadc_search_dev, in the stragglers' re-search of a host-buffer call,
in both paths of the flat PQ table, and its size caps the sub-batches of a host-buffer IVFADC call.  Every case here takes its
budget from tests/chunk_inputs.py (the restatement of csrc/chunk_plan.h that tests/test_chunk_plan_cpu.py compares with the header,
and that names the regime of the formula each case reaches) and asserts:
  - the cut happened: with the handle's profile on, the per-chunk launches -- ivf_filter / merge_refine (or ivf_exact_scan,
    ivf_multi_scan) of the cell-grouped scans, pq_front of the flat table, lut_build / adc_scan / bigk_replay of the generic
    kernels -- number what chunk_inputs predicts, always more than one, and the same call under the default budget launches once;
  - the lists equal the oracle's bit for bit (the round-one lists of a *_dev call, as tests/test_gpu_dev_contract.py compares
    them) and the same call's lists under the default budget;
  - bound_violations() == 0.
The short tails are where the kernels change shape within one call: a one-query chunk through the batch chain, a last chunk below
the 256 items from which fused = -1 takes the cell-grouped scan (the call starts on filter + refine and ends on the generic
kernels, on one stream and one workspace), fewer than 16 queries through the flat table's cell-grouped scan."""
import functools

import numpy as np
import pytest

import chunk_inputs as ci
import dev_contract_inputs as dci
import util
from test_gpu_dev_contract import _assert_round_one, _dev, _search_dev

pytestmark = pytest.mark.gpu

# every option a case may touch, at its default (csrc/internal.h Tuning)
DEFAULTS = {"fused": -1, "fused_kernel": 5, "scan_share": 0, "lut_budget_mb": ci.DEFAULT_MB, "codes_u8": 1, "running_bound": 1,
            "pipeline_batch": 2048, "pipeline_lanes": 4}
KEYS = {"K256": ("300", 256, 5, False), "K1024": ("300", 1024, 5, False), "k600": ("300", 256, 600, False)}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _options(idx, opts, defaults=DEFAULTS):
    for name, value in {**defaults, **opts}.items():
        idx.set_option(name, value)


def _profiled(idx, call):
    idx.profile_enable(True)
    got = call()
    prof = {name: n for name, (n, _) in idx.profile_read().items()}
    idx.profile_enable(False)
    return got, prof


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what + ": differs from the same call under the default budget"


# ---- IVFADC tables ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(name):
    """-> dict(arrays of the table, ot: the oracle's handle, qs: 300 queries, sentinel)"""
    o = dci.oracle()
    if name in ("K256", "K1024", "k600"):
        key = KEYS[name]
        c = dci.case(*key)
        t = {n: c[n] for n in ("coarse", "codebook", "list_off", "ids", "codes")}
        # (the mixed batch: every designed query -- the empty cell, the cells of one, k - 1 and k rows -- among finished corpus rows)
        qs = dci.batches(*key, dci.CASES[key][0])["mixed"][0]
        return dict(t=t, ot=c["ot"], qs=qs, sentinel=c["sentinel"])
    if name == "multi":
        t = util.shape_ivf_tables(25, 5, 256, 32, 8000)
        qs = util.shape_queries(8000, 25, 64)
        sentinel = 1000.0
    else:
        # "long": the K = 256 table's centroids and codebook over 40 000 rows of random codes, 33 000 of them in ONE list: nine
        # units of 4096 rows, more than the cell-grouped scan of the 300-d shape takes
        assert name == "long"
        c = dci.case(*KEYS["K256"])
        rng = np.random.default_rng(31)
        sizes = np.full(64, (40000 - 33000) // 63, np.int64)
        sizes[7] = 33000
        sizes[-1] += 40000 - sizes.sum()
        t = dict(coarse=c["coarse"], codebook=c["codebook"], list_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                 ids=np.arange(1, 40001, dtype=np.int32), codes=rng.integers(0, 256, size=(40000, 12)).astype(np.int16))
        # (the long list's centroid among the queries' eight nearest cells: corpus rows moved towards it)
        qs = (0.5 * c["corpus"][:64] + 0.5 * c["coarse"][7][None, :]).astype(np.float32)
        sentinel = 1000.0
    ot = o.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    return dict(t=dict(t), ot=ot, qs=qs, sentinel=sentinel)


@pytest.fixture(scope="module")
def pins(gpu):
    held = {}

    def get(name):
        if name not in held:
            t = _table(name)["t"]
            lo, hi = ci.IVF_TABLES[name]["max_rows"]
            assert lo <= int(np.diff(np.asarray(t["list_off"])).max()) <= hi, "input: the longest list is outside the bound chunk_inputs states"
            assert np.asarray(t["coarse"]).shape[0] == ci.IVF_TABLES[name]["C"] and np.asarray(t["codebook"]).shape[:2] == (ci.IVF_TABLES[name]["m"], ci.IVF_TABLES[name]["K"])
            held[name] = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
        return held[name]
    yield get
    for idx in held.values():
        idx.close()


@functools.lru_cache(maxsize=None)
def _expected(name, k, W, rule, sentinel):
    """the oracle's account of the table's queries: round-one lists, unfinished, final lists (as dev_contract_inputs.expected)"""
    o, t = dci.oracle(), _table(name)
    one, found, _ = o.ivfadc_search_many(t["ot"], t["qs"], k, W, sentinel=sentinel, found_rule=rule, max_rounds=1, n_threads=8)
    final, _, rounds = o.ivfadc_search_many(t["ot"], t["qs"], k, W, sentinel=sentinel, found_rule=rule, max_rounds=0, n_threads=8)
    return {"round_one": one, "unfinished": found < k, "final": final, "rounds": rounds}


def _rows(exp, rows):
    return {n: exp[n][rows] for n in ("round_one", "unfinished", "final")}


def _scan_counts(case, fused, kernel=5):
    """{launch name: count} the chunks of a *_dev call must show: per chunk the path ivfadc_begin takes for its queries"""
    t = ci.IVF_TABLES[case["table"]]
    grouped_ok = 2 * case["k"] <= 64 and "long" not in case["regime"]
    want = {}
    for _, n in ci.cuts(case["Q"], case["per"]):
        grouped = grouped_ok and (fused == 1 or (fused == -1 and n * case["W"] >= ci.AUTO_ITEMS))
        if grouped:
            names = ("lut_build", "ivf_multi_scan", "merge_surv") if not t["special"] else ("ivf_exact_scan", "merge_surv") if kernel == 3 else ("ivf_filter", "merge_refine")
        else:
            names = ("lut_build", "bigk_replay") if 2 * case["k"] > 1024 else ("lut_build", "adc_scan", "merge_replay")
        for name in names:
            want[name] = want.get(name, 0) + 1
    if 2 * case["k"] > 1024:
        want["adc_scan"] = want["merge_select"] = want["lut_build"] * ci.cdiv(2 * case["k"], 1024)
    want["probe_plan"] = len(ci.cuts(case["Q"], case["per"]))
    return want


ALL_SCANS = ("probe_plan", "ivf_filter", "merge_refine", "ivf_exact_scan", "ivf_multi_scan", "merge_surv", "lut_build", "adc_scan", "merge_replay", "merge_select", "bigk_replay")


def _run_dev(idx, case, fused, rules=(0, 1), opts=None, order=None, kernel=5):
    """one chunked freddy_gpu_ivfadc_search_dev call per found rule, and the same call under the default budget"""
    import torch
    t = _table(case["table"])
    mb = ci.ivf_budget(case)
    Q, k, W = case["Q"], case["k"], case["W"]
    rows = np.arange(Q) if order is None else order
    qs = np.ascontiguousarray(t["qs"][rows])
    want = _scan_counts(case, fused, kernel)
    assert want["probe_plan"] == len(ci.cuts(Q, case["per"])) >= 3
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    verdicts = []
    for rule in rules:
        exp = _rows(_expected(case["table"], k, W, rule, t["sentinel"]), rows)
        what = f"{case['id']} fused={fused} rule={rule} {opts or ''}"
        _options(idx, {"fused": fused, "fused_kernel": kernel, "lut_budget_mb": mb, **(opts or {})})
        gi, gd, status, prof = _search_dev(idx, qs, k, W, t["sentinel"], rule, stream)
        _options(idx, {"fused": fused, "fused_kernel": kernel, **(opts or {})})
        di, dd, dstatus, dprof = _search_dev(idx, qs, k, W, t["sentinel"], rule, stream)
        _options(idx, {})
        print(what, "budget", mb, "chunked", {n: prof.get(n) for n in ALL_SCANS if n in prof}, "default", {n: dprof.get(n) for n in ALL_SCANS if n in dprof})
        assert {n: prof.get(n, 0) for n in ALL_SCANS if n in prof or n in want} == want, (what, want, prof)
        assert dprof.get("probe_plan") == 1, (what, dprof)
        _assert_round_one(gi, gd, exp, what)
        _same((gi, gd), (di, dd), what)
        verdicts.append((what, status, dstatus, bool(exp["unfinished"].any())))
    assert idx.bound_violations() == 0
    for what, status, dstatus, some in verdicts:
        assert (status != 0) == some and (dstatus != 0) == some, f"{what}: status word {status} (default budget: {dstatus}), the oracle says unfinished = {some}"


@pytest.mark.parametrize("fused", [1, 0, -1])
@pytest.mark.parametrize("case", ci.DEV_MATRIX, ids=lambda c: c["id"])
def test_dev_chunk_sizes_with_and_without_a_tail(gpu, pins, case, fused):
    """chunks of 1, 31, 32, 33, 64 and 65 queries (either side of the 32- and 64-query tiles of the cell selection), three full
    ones and a tail of one query, or none.  fused = -1: a chunk of one query (32 items) takes the generic kernels, so from 31
    queries on the call with a tail runs both the cell-grouped and the generic launches."""
    if fused == -1 and case["per"] >= 31 and case["Q"] % 3:
        want = _scan_counts(case, fused)
        assert want["ivf_filter"] == 3 and want["adc_scan"] == 1
    _run_dev(pins("K256"), case, fused)


@pytest.mark.parametrize("fused", [1, 0, -1])
@pytest.mark.parametrize("case", ci.DEV_REGIMES, ids=lambda c: c["id"])
def test_dev_every_regime_of_the_formula(gpu, pins, case, fused):
    """the LUT term (K = 1024), the summed terms of a multi.h shape, 2k > 64, 2k > 1024 and lists too long for survivor regions"""
    _run_dev(pins(case["table"]), case, fused)


MIDDLE_OPTS = [(1, 5, {}), (0, 5, {}), (-1, 5, {}), (1, 3, {}), (1, 5, {"codes_u8": 0}), (1, 5, {"codes_u8": 2}), (1, 5, {"running_bound": 0}),
               (1, 5, {"scan_share": 4})]


@pytest.mark.parametrize("fused,kernel,opts", MIDDLE_OPTS, ids=lambda v: str(v).replace(" ", ""))
def test_dev_unfinished_queries_in_a_middle_chunk(gpu, pins, fused, kernel, opts):
    """the mixed batch's unfinished queries (W = 1) all in the second of four chunks (96, 96, 96, 12): the word is set, the chunks
    before and behind keep their lists; under both found rules, the exact-distance scan, both code layouts and without running bounds"""
    case = ci.DEV_MIDDLE
    t = _table("K256")
    unf = np.zeros(300, bool)
    for rule in (0, 1):
        unf |= _expected("K256", case["k"], 1, rule, t["sentinel"])["unfinished"]
    n_unf = int(unf.sum())
    assert 0 < n_unf <= case["per"]
    fin, late = np.flatnonzero(~unf), np.flatnonzero(unf)
    order = np.concatenate([fin[:case["per"]], late, fin[case["per"]:]])
    at = np.flatnonzero(unf[order])
    assert at.min() >= case["per"] and at.max() < 2 * case["per"], "input: an unfinished query lies outside the second chunk"
    _run_dev(pins("K256"), case, fused, opts=opts, order=order, kernel=kernel)


# ---- the host-buffer IVFADC call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, -1])
@pytest.mark.parametrize("case", ci.HOST_CALLS, ids=lambda c: c["id"])
def test_host_call_sub_batches_within_the_chunk_size(gpu, pins, case, fused):
    """the chunk size caps the sub-batches (pipe_cuts): a cap of ONE query makes nine sub-batches on four lanes of two slots -- the
    ninth reuses a slot, every one is read in place -- and a cap of 33 cuts 100 queries into four of 25"""
    idx, t = pins("K256"), _table("K256")
    Q, k, W = case["Q"], case["k"], case["W"]
    subs = ci.sub_batches(Q, case["per"])
    assert len(subs) >= 3
    exp = _expected("K256", k, W, 0, t["sentinel"])["final"][:Q]
    _options(idx, {"fused": fused, "lut_budget_mb": ci.ivf_budget(case)})
    got, prof = _profiled(idx, lambda: idx.search(t["qs"][:Q], k, W, sentinel=t["sentinel"], found_rule=0))
    _options(idx, {"fused": fused})
    dflt, dprof = _profiled(idx, lambda: idx.search(t["qs"][:Q], k, W, sentinel=t["sentinel"], found_rule=0))
    _options(idx, {})
    print(case["id"], fused, prof, dprof)
    grouped = fused == 1 or subs[0][1] * W >= ci.AUTO_ITEMS
    assert prof.get("ivf_filter" if grouped else "adc_scan") == len(subs) and prof.get("probe_plan") == len(subs), (len(subs), prof)
    assert dprof.get("probe_plan") == 1, dprof
    util.assert_same_lists(got[0], got[1], exp, f"{case['id']} fused={fused}")
    _same(got, dflt, case["id"])
    assert idx.bound_violations() == 0


@pytest.fixture(scope="module")
def thin(gpu):
    """the 600-row, C = 150, K = 64 table of tests/test_gpu_pipeline.py (k = 10, W = 1, the rows rule: a query whose nearest cell holds
    fewer than 10 rows is a straggler): 65 stragglers and 20 finished queries in a seeded order, which the budget of
    chunk_inputs.STRAGGLERS cuts into sub-batches of 29, 29 and 27"""
    from freddy_amd import index_build as ib
    o = dci.oracle()
    s = ci.STRAGGLERS
    x = util.corpus(600)
    t = ib.build_ivf_index(x, C=150, m=12, K=64, train_size=600, iters=3, seed=9)
    xs = x.numpy().astype(np.float32)
    ot = o.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    _, found, _ = o.ivfadc_search_many(ot, xs, s["k"], 1, sentinel=1000.0, found_rule=0, max_rounds=1)
    _, _, rounds = o.ivfadc_search_many(ot, xs, s["k"], 1, sentinel=1000.0, found_rule=0, max_rounds=0)
    late, done = np.flatnonzero(found < s["k"]), np.flatnonzero(found >= s["k"])
    assert late.size >= s["stragglers"] and done.size >= s["Q"] - s["stragglers"]
    rng = np.random.default_rng(3)
    pick = rng.permutation(np.concatenate([late[:s["stragglers"]], done[:s["Q"] - s["stragglers"]]]))
    straggler = np.isin(pick, late)
    exp = o.ivfadc_search_many(ot, xs[pick], s["k"], 1, sentinel=1000.0, found_rule=0)
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    vec = gpu.VectorIndex(np.arange(1, 601, dtype=np.int32), xs)
    assert ci.IVF_TABLES["thin"]["max_rows"][0] <= int(np.diff(np.asarray(t["list_off"])).max()) <= ci.IVF_TABLES["thin"]["max_rows"][1]
    yield dict(idx=idx, vec=vec, xs=xs, pick=pick, qs=np.ascontiguousarray(xs[pick]), exp=exp, rounds=rounds[pick], straggler=straggler)
    vec.close()
    idx.close()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("source", ["pageable", "pinned", "ids"])
def test_host_call_stragglers_of_every_sub_batch(gpu, thin, source, fused):
    """65 stragglers among 85 queries, the budget's sub-batches of 29, 29 and 27: every sub-batch's stragglers are searched again
    (ivfadc_sync_search: one chunk, chunk_inputs.STRAGGLERS says why never more) with their extra probing rounds on the handle's
    stream and workspace, between the round-one chains of the other lanes -- a round per sub-batch for as long as one of ITS
    stragglers is unfinished.  From pageable and pinned queries and from a device source (search_ids: the rows are gathered again)."""
    s, idx = ci.STRAGGLERS, thin["idx"]
    subs = ci.sub_batches(s["Q"], s["per"])
    assert [n for _, n in subs] == [29, 29, 27]
    late = np.where(thin["straggler"], thin["rounds"], 0)
    assert all(late[q0:q0 + n].max() >= 2 for q0, n in subs), "input: a sub-batch without stragglers"
    rounds = len(subs) + sum(int(late[q0:q0 + n].max()) for q0, n in subs)
    rounds_whole = 1 + int(late.max())
    pb = gpu.PinnedBuffer(thin["qs"].shape)
    pb.array[:] = thin["qs"]
    ids = (thin["pick"] + 1).astype(np.int32)

    def call():
        if source == "ids":
            return idx.search_ids(thin["vec"], ids, s["k"], 1, sentinel=1000.0, found_rule=gpu.FOUND_ROWS, rule=gpu.QIDS_POSITIONAL)[1:]
        return idx.search(thin["qs"] if source == "pageable" else pb.array, s["k"], 1, sentinel=1000.0, found_rule=gpu.FOUND_ROWS)
    _options(idx, {"fused": fused, "lut_budget_mb": ci.ivf_budget(s)})
    got, prof = _profiled(idx, call)
    _options(idx, {"fused": fused})
    dflt, dprof = _profiled(idx, call)
    _options(idx, {})
    print(source, fused, "rounds", rounds, rounds_whole, prof, dprof)
    scan = "ivf_filter" if fused else "adc_scan"
    assert prof.get(scan) == rounds > rounds_whole and dprof.get(scan) == rounds_whole, (rounds, rounds_whole, prof, dprof)
    util.assert_same_lists(got[0], got[1], thin["exp"], f"stragglers, {source}, fused={fused}")
    _same(got, dflt, f"stragglers, {source}")
    assert idx.bound_violations() == 0
    pb.close()


# ---- the flat PQ table ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pq_table(N, n_distinct=100000):
    """a random codebook and rows drawn from a pool of code rows (7: the duplicate-heavy pool of test_soak_random_pq_table), 241
    queries: the one at 16 lies beyond the sentinel 100.0"""
    rng = np.random.default_rng(700 + N + n_distinct)
    codebook = (rng.standard_normal((ci.PQ_M, ci.PQ_K, 25)) * 0.3).astype(np.float32)
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    pool = rng.integers(0, ci.PQ_K, size=(n_distinct, ci.PQ_M)).astype(np.int16)
    codes = pool[rng.integers(0, n_distinct, size=N)]
    qs = (0.5 * rng.standard_normal((241, 300))).astype(np.float32)
    qs[16] *= np.float32(40.0)
    sub = rng.choice(ids, size=ci.PQ_SUBSET_ROWS, replace=False).astype(np.int32) if N >= ci.PQ_SUBSET_ROWS else None
    return dict(codebook=codebook, ids=ids, codes=codes, qs=qs, ot=dci.oracle().pq_table(codebook, ids, codes), sub=sub)


@functools.lru_cache(maxsize=None)
def _pq_expected(N, n_distinct, k, Q):
    t = _pq_table(N, n_distinct)
    o = dci.oracle()
    return np.stack([o.pq_search(t["ot"], q, k) for q in t["qs"][:Q]])


@pytest.fixture(scope="module")
def pq_pins(gpu):
    held = {}

    def get(N, n_distinct=100000):
        if (N, n_distinct) not in held:
            t = _pq_table(N, n_distinct)
            held[(N, n_distinct)] = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
        return held[(N, n_distinct)]
    yield get
    for idx in held.values():
        idx.close()


PQ_DEFAULTS = {"pq_fused": -1, "lut_budget_mb": ci.DEFAULT_MB}


def _pq_counts(case, chunks):
    if case["fused"]:
        return {"pq_front": chunks, "ivf_filter": chunks, "merge_refine": chunks}
    if 2 * case["k"] > 1024:
        return {"lut_build": chunks, "adc_scan": chunks * ci.cdiv(2 * case["k"], 1024), "bigk_replay": chunks}
    return {"lut_build": chunks, "adc_scan": chunks, "merge_replay": chunks}


def _pq_dev_call(idx, qs, k, sentinel):
    import torch
    dq, oi, od, _ = _dev(qs, k)
    idx.search_dev(dq.data_ptr(), qs.shape[0], k, sentinel, oi.data_ptr(), od.data_ptr(), None)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy()


def _run_pq(idx, case, exp, call, n_blocks, what):
    chunks = len(ci.cuts(case["Q"], case["per"]))
    want = _pq_counts(case, chunks)
    assert chunks >= 3
    _options(idx, {"pq_fused": case["fused"], "lut_budget_mb": ci.pq_budget(case, n_blocks)}, PQ_DEFAULTS)
    got, prof = _profiled(idx, call)
    _options(idx, {"pq_fused": case["fused"]}, PQ_DEFAULTS)
    dflt, dprof = _profiled(idx, call)
    _options(idx, {}, PQ_DEFAULTS)
    print(what, "chunked", prof, "default", dprof)
    assert {n: prof.get(n) for n in want} == want, (what, want, prof)
    assert {n: dprof.get(n) for n in want} == _pq_counts(case, 1), (what, dprof)
    assert ("pq_front" in prof) == bool(case["fused"]) and ("lut_build" in prof) == (not case["fused"]), (what, prof)
    util.assert_same_lists(got[0], got[1], exp, what)
    _same(got, dflt, what)
    assert idx.bound_violations() == 0


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("case", ci.PQ_CALLS, ids=lambda c: c["id"])
def test_pq_call_in_chunks(gpu, pq_pins, case, entry):
    """both paths of the flat table through freddy_gpu_pq_search and freddy_gpu_pq_search_dev: chunks of 16 queries through the
    cell-grouped scan with tails of 1 and 2 (pq_use_fused is decided on the call's Q: the automatic mode never sends fewer than 16
    there) and chunks of 19 and 48; the generic scan with k = 32 and, per chunk, the selection passes of k = 600"""
    t = _pq_table(case["N"])
    idx = pq_pins(case["N"])
    qs = np.ascontiguousarray(t["qs"][:case["Q"]])
    exp = _pq_expected(case["N"], 100000, case["k"], case["Q"])
    assert (exp["id"][16] == -1).all() and (exp["id"][0] >= 0).all(), "input: the query beyond the sentinel"
    call = (lambda: idx.search(qs, case["k"], sentinel=100.0)) if entry == "host" else (lambda: _pq_dev_call(idx, qs, case["k"], 100.0))
    _run_pq(idx, case, exp, call, ci.blocks_of(case["N"]), f"{case['id']} {entry}")


@pytest.mark.parametrize("case", [ci.PQ_CALLS[0], ci.PQ_CALLS[6]], ids=lambda c: c["id"])
def test_pq_duplicate_heavy_table_in_chunks(gpu, pq_pins, case):
    """40 000 rows drawn from SEVEN code rows: every list position is decided by the order of equal keys, in every chunk"""
    t = _pq_table(case["N"], 7)
    idx = pq_pins(case["N"], 7)
    qs = np.ascontiguousarray(t["qs"][:case["Q"]])
    _run_pq(idx, case, _pq_expected(case["N"], 7, case["k"], case["Q"]), lambda: idx.search(qs, case["k"], sentinel=100.0), ci.blocks_of(case["N"]),
            f"{case['id']} duplicates")


@pytest.mark.parametrize("case", ci.PQ_SUBSETS, ids=lambda c: c["id"])
def test_pq_subset_chunks_follow_the_subset(gpu, pq_pins, case):
    """subset_ids of 5000 rows (79 row blocks, two pseudo-lists): the chunk size takes the SUBSET's row blocks -- the table's 625
    would cut the call into another number of chunks (tests/test_chunk_plan_cpu.py)"""
    t = _pq_table(case["N"])
    idx = pq_pins(case["N"])
    qs = np.ascontiguousarray(t["qs"][:case["Q"]])
    exp = dci.oracle().pq_search_in_batch(t["ot"], qs, case["k"], t["sub"], use_target_lists=True)
    _run_pq(idx, case, exp, lambda: idx.search(qs, case["k"], sentinel=1000.0, subset_ids=t["sub"]), ci.blocks_of(ci.PQ_SUBSET_ROWS), case["id"])


# ---- the entry points layered on the chunked calls ----------------------------------------------------------------------------------------
# Each does its own gathers, id mapping or per-device split around the chunk loop: one chunked call each on pv_model.main_tables()
# (20 000 x 300, C = 32, K = 256), against the oracle-only models the entry points' own tests use and against the default budget.
@pytest.fixture(scope="module")
def layers(gpu):
    import pv_model as pm
    o = dci.oracle()
    x, ids, qs, ivf, pq = pm.main_tables()
    args = (ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    lo, hi = ci.IVF_TABLES["main"]["max_rows"]
    assert lo <= int(np.diff(np.asarray(ivf["list_off"])).max()) <= hi and np.asarray(ivf["coarse"]).shape[0] == ci.IVF_TABLES["main"]["C"]
    assert len(pq["ids"]) == ci.LAYERS_PQ["N"]
    rng = np.random.default_rng(12)
    texts = []
    for i in range(100):   # every ninth text is empty, every eleventh holds ids without a row only
        t = rng.choice(ids, size=int(rng.integers(1, 7))).astype(np.int32)
        texts.append(np.empty(0, np.int32) if i % 9 == 0 else (t + 10 ** 6).astype(np.int32) if i % 11 == 0 else t)
    h = dict(x=x, ids=ids, qs=qs, texts=texts, rows=np.arange(0, 20000, 283)[:70],
             ivf=gpu.IVFIndex(*args), twice=gpu.IVFIndex(*args, devices=[0, 0]), pq=gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"]),
             vec=gpu.VectorIndex(ids, x), ivf_t=o.ivf_table(*args), pq_t=o.pq_table(pq["codebook"], pq["ids"], pq["codes"]))
    yield h
    for n in ("ivf", "twice", "pq", "vec"):
        h[n].close()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _layer(idx, opts, defaults, call, count, want, what):
    """call() under the budget of `opts` and under the default one: `count` launches `want` (> 1) times, then once; equal outputs"""
    assert want >= 3
    _options(idx, opts, defaults)
    got, prof = _profiled(idx, call)
    _options(idx, {k: v for k, v in opts.items() if k != "lut_budget_mb"}, defaults)
    dflt, dprof = _profiled(idx, call)
    _options(idx, {}, defaults)
    print(what, "chunked", prof, "default", dprof)
    assert prof.get(count) == want and dprof.get(count) == 1, (what, want, prof, dprof)
    assert len(got) == len(dflt) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, dflt)), what + ": differs from the same call under the default budget"
    assert idx.bound_violations() == 0
    return got


def _texts_expected(h, search):
    """the text vectors (freddy_gpu_tokenize, which tests/test_gpu_tokenize.py compares with its model) through the oracle's search"""
    vecs_of, counts = h["vec"].tokenize(h["texts"])
    live = counts > 0
    assert 0 < live.sum() < live.size
    return counts, live, search(np.ascontiguousarray(vecs_of[live]))


def _same_texts(got, counts, live, exp, filler, what):
    gc, gi, gd = got
    assert np.array_equal(gc, counts), what
    util.assert_same_lists(gi[live], gd[live], exp, what)
    assert (gi[~live] == -1).all() and (gd[~live] == np.float32(filler)).all(), what + ": fillers"


@pytest.mark.parametrize("fused", [-1, 1])
@pytest.mark.parametrize("entry", ["search_pv", "search_ids", "search_texts", "analogy", "two_devices"])
def test_ivfadc_entry_points_over_a_cut_call(gpu, layers, entry, fused):
    """sub-batches of at most 21 queries (W = 3: 96 KiB per query) under search_pv at k x pvf = 30, search_ids (rows gathered on the
    device), search_texts (the live texts' vectors stay on the device), the approximate analogies' search at n_cand = 23, and a
    handle of two replicas, whose first half of the batch is cut again (the profile is the first replica's)"""
    import approx_analogy_model as am
    import pv_model as pm
    h, o, case = layers, dci.oracle(), ci.LAYERS_IVF
    ivf, vec, x, ids, qs, W = h["ivf"], h["vec"], h["x"], h["ids"], h["qs"], case["W"]
    opts = {"fused": fused, "lut_budget_mb": ci.ivf_budget(case)}
    subs = lambda n: len(ci.sub_batches(n, case["per"]))
    what = f"ivfadc {entry} fused={fused}"
    if entry == "search_pv":
        Q = case["Q"]
        exp, _, _ = pm.expected(o, pm.ivf_lists(o, h["ivf_t"], qs[:Q], 30, W), x, ids, qs[:Q], 5)
        gi, gs = _layer(ivf, opts, DEFAULTS, lambda: ivf.search_pv(vec, qs[:Q], 5, 6, W), "probe_plan", subs(Q), what)
        pm.same(gi, gs, exp, 5, what)
    elif entry == "search_ids":
        rows = h["rows"]
        exp = o.ivfadc_search_many(h["ivf_t"], x[rows], 5, W, sentinel=1000.0, found_rule=0, n_threads=8)
        gq, gi, gd = _layer(ivf, opts, DEFAULTS, lambda: ivf.search_ids(vec, ids[rows], 5, W, rule=gpu.QIDS_POSITIONAL), "probe_plan", subs(rows.size), what)
        assert np.array_equal(gq, ids[rows])
        util.assert_same_lists(gi, gd, exp, what)
    elif entry == "search_texts":
        counts, live, exp = _texts_expected(h, lambda v: o.ivfadc_search_many(h["ivf_t"], v, 5, W, sentinel=1000.0, found_rule=0, n_threads=8))
        got = _layer(ivf, opts, DEFAULTS, lambda: ivf.search_texts(vec, h["texts"], 5, W), "probe_plan", subs(int(live.sum())), what)
        _same_texts(got, counts, live, exp, 1000.0, what)
    elif entry == "analogy":
        triples = am.main_triples()
        exp, stats = am.ivf_expected(o, h["ivf_t"], x, ids, triples, 5, 23, W)[:2]
        assert stats["searched"] == len(triples)
        gi, gs = _layer(ivf, opts, DEFAULTS, lambda: ivf.analogy(vec, triples, k=5, n_cand=23, W=W), "probe_plan", subs(len(triples)), what)
        pm.same(gi, gs, exp, 5, what)
    else:
        twice, Q = h["twice"], 2 * case["Q"]
        assert twice.replicas == 2
        exp = o.ivfadc_search_many(h["ivf_t"], qs[:Q], 5, W, sentinel=1000.0, found_rule=0, n_threads=8)
        gi, gd = _layer(twice, opts, DEFAULTS, lambda: twice.search(qs[:Q], 5, W), "probe_plan", subs(Q // 2), what)
        util.assert_same_lists(gi, gd, exp, what)


@pytest.mark.parametrize("entry", ["search_pv", "search_ids", "search_texts", "analogy"])
def test_pq_entry_points_over_a_cut_call(gpu, layers, entry):
    """the flat table of 20 000 rows in chunks of 32 queries through the cell-grouped scan, under the same entry points"""
    import approx_analogy_model as am
    import pv_model as pm
    h, o, case = layers, dci.oracle(), ci.LAYERS_PQ
    pq, vec, x, ids, qs = h["pq"], h["vec"], h["x"], h["ids"], h["qs"]
    opts = {"lut_budget_mb": ci.pq_budget(case, ci.blocks_of(case["N"]))}
    chunks = lambda n: len(ci.cuts(n, case["per"]))
    search = lambda v, k: np.stack([o.pq_search(h["pq_t"], q, k) for q in v])
    what = f"pq {entry}"
    if entry == "search_pv":
        Q = case["Q"]
        exp, _, _ = pm.expected(o, pm.pq_lists(o, h["pq_t"], qs[:Q], 30), x, ids, qs[:Q], 5)
        gi, gs = _layer(pq, opts, PQ_DEFAULTS, lambda: pq.search_pv(vec, qs[:Q], 5, 6), "pq_front", chunks(Q), what)
        pm.same(gi, gs, exp, 5, what)
    elif entry == "search_ids":
        rows = h["rows"]
        gq, gi, gd = _layer(pq, opts, PQ_DEFAULTS, lambda: pq.search_ids(vec, ids[rows], 5, rule=gpu.QIDS_POSITIONAL), "pq_front", chunks(rows.size), what)
        assert np.array_equal(gq, ids[rows])
        util.assert_same_lists(gi, gd, search(x[rows], 5), what)
    elif entry == "search_texts":
        counts, live, exp = _texts_expected(h, lambda v: search(v, 5))
        got = _layer(pq, opts, PQ_DEFAULTS, lambda: pq.search_texts(vec, h["texts"], 5), "pq_front", chunks(int(live.sum())), what)
        _same_texts(got, counts, live, exp, 100.0, what)
    else:
        triples = am.main_triples()
        exp, stats = am.pq_expected(o, h["pq_t"], x, ids, triples, 5, 23)[:2]
        assert stats["searched"] == len(triples)
        gi, gs = _layer(pq, opts, PQ_DEFAULTS, lambda: pq.analogy(vec, triples, k=5, n_cand=23), "pq_front", chunks(len(triples)), what)
        pm.same(gi, gs, exp, 5, what)


# ---- reserve_cus -----------------------------------------------------------------------------------------------------------------------------
GRID_DEFAULTS = {**DEFAULTS, "reserve_cus": 0, "scan_elastic": 0, "grid_cus": 0}


@pytest.mark.parametrize("elastic", [0, 1])
@pytest.mark.parametrize("share", [1, 4])
@pytest.mark.parametrize("reserve", [0, 2, 400])
def test_reserved_cus_on_a_handful_of_cus(gpu, pins, reserve, share, elastic):
    """option reserve_cus (CUs the persistent scans leave to other streams) on a handle limited to seven CUs: with two reserved and
    four batches sharing, and with more reserved than the device has, scan_cus and filter_scan_cap (csrc/grid_plan.h) are negative
    and the grids rest on their clamps -- one workgroup that pulls every entry.  Both filter scans (codes_u8 = 1: the whole slab in
    LDS; 2: the one that brings elastic extras), a device-pointer and a host-buffer call each; lists equal the oracle's."""
    import torch
    import grid_inputs as gi_
    n_cus = 7
    assert reserve <= 2 or reserve > gi_.DEVICE_CUS
    own, cap = max(n_cus // share, min(n_cus, 32)) - reserve, n_cus - 64 - reserve * share
    assert cap < 0 and (own < 0) == (reserve == 400) and own == gi_._scan_cus(n_cus, share, reserve)
    idx, t = pins("K256"), _table("K256")
    k, W, Q = 5, 4, 150
    qs = np.ascontiguousarray(t["qs"][:Q])
    exp = _rows(_expected("K256", k, W, 0, t["sentinel"]), np.arange(Q))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for codes_u8 in (1, 2):
        what = f"reserve_cus={reserve} scan_share={share} scan_elastic={elastic} codes_u8={codes_u8}"
        _options(idx, {"fused": 1, "codes_u8": codes_u8, "scan_share": share, "scan_elastic": elastic, "reserve_cus": reserve, "grid_cus": n_cus}, GRID_DEFAULTS)
        gi, gd, status, prof = _search_dev(idx, qs, k, W, t["sentinel"], 0, stream)
        hi, hd = idx.search(qs, k, W, sentinel=t["sentinel"], found_rule=0)
        _options(idx, {}, GRID_DEFAULTS)
        assert prof.get("ivf_filter") == 1 and "adc_scan" not in prof, (what, prof)
        _assert_round_one(gi, gd, exp, what)
        assert (status != 0) == bool(exp["unfinished"].any()), what
        util.assert_same_lists(hi, hd, exp["final"], what + ": host-buffer call")
    assert idx.bound_violations() == 0
