"""-m gpu: ivf_filter5_kernel's selection tail in two item segments (fused5.h, scan_tail5.inc).

An entry of more than 8 items runs its tail in two segments, items 0-7 and 8-15, with the thresholds of one segment sorted by the
builder waves while the gatherer waves work on the other, and one barrier more than an entry of up to 8 items.  What can go wrong
is decided by the ITEM COUNT of an entry (either side of 8, a full and a partly filled second segment, a second entry of the same
cell from 17 items on) and by the rows of its chunk (a partly filled last block, a second chunk that is nearly empty).

The index has two cells and every query probes both, so a cell's item count is the batch size: Q = 1 .. 25.  Cell 0 holds 70 rows
(two blocks, the second with 6 rows), cell 1 holds 4096 + 65 (a full chunk and one of two blocks, the second with one row).

Ties: a gatherer lane holds the rows of its chunk that lie 512 apart (row j: block j / 64 of wave (j / 64) % 8, lane j % 64), so the
first 600 rows of cell 1 carry ONE code row -- rows j and j + 512, j < 88, are two equal sums in one lane -- and that code row is
the one of a table row whose vector is two queries out of three of every batch (index i with i % 3 != 1).  For those queries the
600 rows are the nearest of the cell at one distance: all of them are at or below the threshold, and the lanes j < 88 take the
two-survivors path of the survivor pass.  Which slot of an entry a query gets is the work table's business; with 11 of 16 queries
such copies a full entry (Q = 16, 17, 25) has some in items 0-7 AND in items 8-15 whatever the order.  The first 40 rows of cell 0
share a code row too (equal distances in different lanes).  K = 1024 is the FULLK instantiation, K = 256 with codes_u8 = 0 and 2 the other
two; codes_u8 = 1 (ivf_filter8_kernel, which includes the same text with its default range) is checked too.  Every list is compared
with the CPU oracle's bit for bit, and no refined row may leave its bracket."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

D, M, C, W = 300, 12, 2, 2
ROWS = (70, 4096 + 65)
N = sum(ROWS)
BATCHES = (1, 4, 5, 8, 9, 12, 16, 17, 25)
VARIANTS = ((1024, 1), (256, 0), (256, 2), (256, 1))     # (K, codes_u8)
CALLS = ((5, 0, 1000.0), (5, 1, 100.0))                  # (k, found rule, sentinel): CAND off and on
DUP = (40, 600)                                           # rows at the head of each list with one code row (cell 1: past 512)


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def index(gpu, oracle):
    """K -> (oracle table, handle, 25 queries, {(Q, k, rule, sentinel): the oracle's lists}); built on first use"""
    made = {}

    def get(K):
        if K not in made:
            t = dict(util.shape_ivf_tables(D, M, K, C, N))
            # the same rows, cut into lists of 70 and 4161 (both sides read these arrays: which centroid a row's codes were made
            # for does not matter to either)
            # cell 1's shared code row: that of a row the index put into cell 1 (its codes go with coarse[1]), whose vector is a query
            src = max(int(t["list_off"][1]), ROWS[0])
            tie_query = util.shape_corpus(N, D)[int(t["ids"][src]) - 1].numpy().astype(np.float32)
            t["list_off"] = np.array([0, ROWS[0], N], np.int32)
            t["ids"] = (np.arange(N) * 3 + 2).astype(np.int32)      # (ascending inside a list, as a pin wants them)
            codes = t["codes"].copy()
            codes[0:DUP[0]] = codes[0]
            codes[ROWS[0]:ROWS[0] + DUP[1]] = t["codes"][src]
            t["codes"] = codes
            qs = util.shape_queries(N, D, max(BATCHES), seed=3).copy()
            qs[np.arange(len(qs)) % 3 != 1] = tie_query
            ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
            idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
            idx.set_option("fused", 1)            # (a few items: below what takes the cell-grouped scans by itself)
            idx.set_option("sparse_items", 0)     # (a cell that one or two queries probe stays a work entry)
            idx.set_option("one_launch", 0)       # (a single query takes the batch's chain too)
            made[K] = (ot, idx, qs, {})
        return made[K]
    yield get
    for _, idx, _, _ in made.values():
        idx.close()


def _expected(oracle, entry, Q, k, rule, sent, qs=None, tag=""):
    ot, _, q0, cache = entry
    key = (Q, k, rule, sent, tag)
    if key not in cache:
        cache[key] = oracle.ivfadc_search_many(ot, q0[:Q] if qs is None else qs, k, W, sentinel=sent, found_rule=rule).reshape(Q, k)
    return cache[key]


def _reset(idx):
    for name, v in (("codes_u8", 1), ("scan_share", 0), ("check_brackets", 0), ("running_bound", 1)):
        idx.set_option(name, v)


def _names(idx, call):
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


@pytest.mark.parametrize("K,u8", VARIANTS)
@pytest.mark.parametrize("share", [0, 4])
def test_item_counts_either_side_of_a_segment(index, oracle, K, u8, share):
    """Q items per cell for every Q of BATCHES, both found-row rules; scan_share = 4: the grid and the merge of batches in flight."""
    entry = index(K)
    idx, qs = entry[1], entry[2]
    _reset(idx)
    idx.set_option("codes_u8", u8)
    idx.set_option("scan_share", share)
    for Q in BATCHES:
        for k, rule, sent in CALLS:
            exp = _expected(oracle, entry, Q, k, rule, sent)
            (gi, gd), names = _names(idx, lambda: idx.search(qs[:Q], k, W, sentinel=sent, found_rule=rule))
            what = f"K={K} codes_u8={u8} scan_share={share} Q={Q} k={k} rule={rule}"
            assert "ivf_filter" in names and "sparse_items" not in names, (what, sorted(names))
            util.assert_exact_lists(gi, gd, exp, k, what)
    assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K,u8", VARIANTS)
def test_every_row_kept_and_refined(index, oracle, K, u8):
    """check_brackets = 1: every threshold is +inf, every row of every item a survivor -- the per-row path of the survivor pass in
    both segments, full regions; the merge refines exactly the rows scanned."""
    entry = index(K)
    idx, qs = entry[1], entry[2]
    _reset(idx)
    idx.set_option("codes_u8", u8)
    idx.set_option("check_brackets", 1)
    for Q in (8, 9, 17):
        exp = _expected(oracle, entry, Q, 5, 0, 1000.0)
        before = idx.bound_checked()
        gi, gd = idx.search(qs[:Q], 5, W, sentinel=1000.0, found_rule=0)
        util.assert_exact_lists(gi, gd, exp, 5, f"every row K={K} codes_u8={u8} Q={Q}")
        checked, rows = idx.bound_checked() - before, idx.last_scanned_rows()
        assert checked == rows > 0, f"K={K} codes_u8={u8} Q={Q}: {checked} brackets checked, {rows} rows scanned"
    assert idx.bound_violations() == 0
    _reset(idx)


@pytest.mark.parametrize("K,u8", [(1024, 1), (256, 0), (256, 2)])
def test_two_streams_with_item_counts_either_side_of_eight(index, oracle, gpu, K, u8):
    """Two different batches of 7 and 12 queries interleaved on two streams with scan_share = 4: entries with and without a second
    segment in flight together; the lists of the same searches run alone."""
    import torch
    dev = torch.device("cuda", 0)
    entry = index(K)
    idx, qs = entry[1], entry[2]
    _reset(idx)
    idx.set_option("codes_u8", u8)
    idx.set_option("scan_share", 4)
    k = 5
    batches = [np.ascontiguousarray(qs[:7]), np.ascontiguousarray(qs[7:19][::-1] * np.float32(1.01))]
    exp = [_expected(oracle, entry, len(b), k, 0, 1000.0, qs=b, tag=f"stream{i}") for i, b in enumerate(batches)]
    dq = [torch.from_numpy(b).to(dev) for b in batches]
    res = [torch.zeros((2, len(b), k), dtype=torch.int32, device=dev) for b in batches]
    st = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in batches]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize(dev)
    for _ in range(6):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                res[i].zero_()
                idx.search_dev(dq[i].data_ptr(), len(batches[i]), k, W, 1000.0, gpu.FOUND_ROWS, res[i][0].data_ptr(), res[i][1].data_ptr(),
                               st[i].data_ptr(), streams[i].cuda_stream)
    torch.cuda.synchronize(dev)
    for i in (0, 1):
        util.assert_exact_lists(res[i][0].cpu().numpy(), res[i][1].view(torch.float32).cpu().numpy(), exp[i], k, f"K={K} codes_u8={u8} stream {i}")
    assert idx.bound_violations() == 0
    _reset(idx)
