"""The elastic scan (option scan_elastic; DESIGN.md 5.1, fused5.h ivf_filter5_elastic_kernel): with scan_share > 1 a scan's grid
brings EXTRA workgroups beyond its n_cus / share guaranteed ones.  An extra takes work entries only while no other scan is announced and
fewer than the cap of scan workgroups are alive, and leaves when one is.  Whatever the extras do, every work entry is scanned exactly
once: every case compares lists and distance bits with the CPU oracle, no bracket is violated, and once the device has drained the
handle's advisory words `active` and `pending` are back at 0.

One small index (d = 300, m = 12, K = 1024, C = 256, 60 000 rows), 512 queries, W = 8, k = 5: about 16 items per cell, more work
entries than the 64 guaranteed workgroups of scan_share = 4, so extras have work."""
import functools

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

N, C, K, Q, W, KNN = 60000, 256, 1024, 512, 8, 5


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@functools.lru_cache(maxsize=None)
def _queries(seed, n=Q):
    return util.queries_from_corpus(N, n, seed=seed)[1]


@functools.lru_cache(maxsize=None)
def _expected(oracle, seed, n=Q):
    """(final lists, round-one lists, found) of the oracle for the batch of `seed` (computed once, shared, never written to)."""
    t = util.ivf_tables(N=N, C=C, K=K)
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    qs = _queries(seed, n)
    exp = oracle.ivfadc_search_many(ot, qs, KNN, W, sentinel=1000.0, found_rule=0, n_threads=8)
    one, found, _ = oracle.ivfadc_search_many(ot, qs, KNN, W, sentinel=1000.0, found_rule=0, max_rounds=1, n_threads=8)
    return exp, one, found


@pytest.fixture(scope="module")
def index(gpu):
    t = util.ivf_tables(N=N, C=C, K=K)
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx.set_option("fused", 1)   # (the cell-grouped scan for the eight-query batch too)
    yield idx
    idx.close()


def _assert_dev_contract(res, status, exp, one, found, what):
    """freddy_gpu_ivfadc_search_dev: the oracle's lists after ONE probing round, final for a query with found >= k; the status word
    is non-zero iff some query is unfinished."""
    import torch
    gi, gd = res[0].cpu().numpy(), res[1].view(torch.float32).cpu().numpy()
    util.assert_same_lists(gi, gd, one, what + ": round-one lists")
    fin = found >= KNN
    util.assert_same_lists(gi[fin], gd[fin], {"id": exp["id"].reshape(gi.shape)[fin], "dist": exp["dist"].reshape(gd.shape)[fin]},
                           what + ": final lists of the finished queries")
    assert (status != 0) == bool((~fin).any()), f"{what}: status word {status}"


class _Batch:
    """One batch on a stream of its own: device buffers of the queries, the lists and the status word."""

    def __init__(self, seed, n=Q):
        import torch
        self.dev = torch.device("cuda", 0)
        self.seed, self.n = seed, n
        self.dq = torch.from_numpy(_queries(seed, n)).to(self.dev)
        self.res = torch.zeros((2, n, KNN), dtype=torch.int32, device=self.dev)
        self.st = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self.stream = torch.cuda.Stream(self.dev)

    def args(self):
        return (self.dq.data_ptr(), self.n, KNN, W, 1000.0, 0, self.res[0].data_ptr(), self.res[1].data_ptr(), self.st.data_ptr(),
                self.stream.cuda_stream)

    def enqueue(self, idx):
        import torch
        with torch.cuda.stream(self.stream):
            self.res.zero_()
            self.st.zero_()
            idx.search_dev(*self.args())

    def check(self, oracle, what):
        exp, one, found = _expected(oracle, self.seed, self.n)
        _assert_dev_contract(self.res, int(self.st[0].item()), exp, one, found, what)


def _options(idx, share, elastic, reserve=64):
    idx.set_option("scan_share", share)
    idx.set_option("scan_elastic_reserve", reserve)
    idx.set_option("scan_elastic", elastic)


def _run_one(idx, oracle, batch, what):
    """One search on an idle chip -> what it added to (started, yielded); active and pending are back at 0."""
    import torch
    before = idx.scan_elastic_stats()
    batch.enqueue(idx)
    torch.cuda.synchronize(batch.dev)
    after = idx.scan_elastic_stats()
    batch.check(oracle, what)
    assert after["active"] == 0 and after["pending"] == 0, f"{what}: {after}"
    assert idx.bound_violations() == 0
    return after["started"] - before["started"], after["yielded"] - before["yielded"]


def test_extras_take_work_on_an_idle_chip(gpu, oracle, index):
    _options(index, 4, 1)
    started, yielded = _run_one(index, oracle, _Batch(41), "elastic, idle chip")
    print(f"started {started} yielded {yielded}")
    assert started > 0


def test_forced_yield_loses_no_entry(gpu, oracle, index):
    """scan_elastic = 2: every extra leaves after its first entry."""
    _options(index, 4, 2)
    started, yielded = _run_one(index, oracle, _Batch(41), "forced yield")
    print(f"started {started} yielded {yielded}")
    assert yielded == started > 0


def test_declined_extras_lose_no_entry(gpu, oracle, index):
    """A reserve of every CU: the cap is not above the guaranteed workgroups, no extra starts."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    _options(index, 4, 1, reserve=n_cus)
    started, yielded = _run_one(index, oracle, _Batch(41), "cap below the guaranteed workgroups")
    assert started == 0 and yielded == 0


def test_fewer_entries_than_guaranteed_workgroups(gpu, oracle, index):
    """Eight queries: guaranteed workgroups without an entry leave at once, extras find the work counter beyond the table."""
    _options(index, 4, 1)
    _run_one(index, oracle, _Batch(43, n=8), "eight queries")


def test_four_streams_interleaved(gpu, oracle, index):
    """Four batches on four streams, twelve interleaved steps: the scans announce themselves to each other's extras."""
    import torch
    _options(index, 4, 1)
    batches = [_Batch(50 + i, n=400) for i in range(4)]
    torch.cuda.synchronize(batches[0].dev)
    before = index.scan_elastic_stats()
    for step in range(12):
        batches[step % 4].enqueue(index)
    torch.cuda.synchronize(batches[0].dev)
    after = index.scan_elastic_stats()
    print(f"started {after['started'] - before['started']} yielded {after['yielded'] - before['yielded']}")
    for i, b in enumerate(batches):
        b.check(oracle, f"four streams, stream {i}")
    assert after["active"] == 0 and after["pending"] == 0, after
    assert index.bound_violations() == 0


def test_second_probing_round_tiny_cells(gpu, oracle):
    """Cells with fewer than k rows and the found-rows rule force further probing rounds (tests/test_gpu_parity.py
    test_ivfadc_multi_round_tiny_cells); codes_u8 = 0 sends the K = 64 table through the six-phase scan, the one that has extras."""
    from freddy_amd import index_build as ib
    n = 600
    x = util.corpus(n)
    t = ib.build_ivf_index(x, C=150, m=12, K=64, train_size=n, iters=3, seed=9)
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx.set_option("fused", 1)
    idx.set_option("codes_u8", 0)
    _options(idx, 4, 1)
    qs = x.numpy()[::7].astype(np.float32)
    for w, k in ((1, 10), (2, 25)):
        gi, gd = idx.search(qs, k, w, sentinel=1000.0, found_rule=gpu.FOUND_ROWS)
        exp = oracle.ivfadc_search_many(ot, qs, k, w, sentinel=1000.0, found_rule=0)
        util.assert_same_lists(gi, gd, exp, f"multi-round W={w} k={k}")
    st = idx.scan_elastic_stats()
    assert st["active"] == 0 and st["pending"] == 0, st
    assert idx.bound_violations() == 0
    idx.close()


def test_graph_replay(gpu, oracle, index):
    """The *_dev call captured into a graph with elasticity on, replayed three times: the record launch's announcement and the
    scan's bookkeeping are part of the graph and balance on every replay."""
    import torch
    _options(index, 4, 1)
    b = _Batch(47)
    call = index.bind_search_dev(*b.args())
    call()                                  # (the stream's workspace is allocated by its first search)
    torch.cuda.synchronize(b.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=b.stream):
        call()
    for n in range(3):
        b.res.zero_()
        b.st.zero_()
        torch.cuda.synchronize(b.dev)
        with torch.cuda.stream(b.stream):
            g.replay()
        torch.cuda.synchronize(b.dev)
        b.check(oracle, f"graph replay {n}")
        st = index.scan_elastic_stats()
        assert st["active"] == 0 and st["pending"] == 0, st
    assert index.bound_violations() == 0
    del g


def test_share_one_has_no_extras(gpu, oracle, index):
    """scan_share = 1: the whole chip is the scan's own, as before -- the option changes nothing."""
    _options(index, 1, 1)
    started, yielded = _run_one(index, oracle, _Batch(41), "scan_share 1")
    assert started == 0 and yielded == 0
    _options(index, 0, 0)
