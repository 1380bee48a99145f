"""-m gpu: NaN, -NaN and +-Inf in queries, codebooks, coarse centroids and raw rows on every search path.

Every batch is compared with the CPU oracle bit for bit -- the poisoned queries' lists too (tests/test_nonfinite_cpu.py pins
what the oracle answers) -- and every healthy query's list with the list the SAME call gives when the poisoned queries are
replaced by finite ones: a poisoned neighbour in the same tile, cell, work entry or wave must change nothing.  The path of
each case is forced with the switches of tests/test_gpu_parity.py and read back from the handle's profile.  The self-check
counters must stay at zero, also with every row / every cell sent through the exact stage ("Non-finite
inputs": a row or cell whose reference value or bracket is not finite is not counted)."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
Q = 136        # two query tiles of 64 and a ragged third; 17 groups of 8


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


def _ivf_expect(oracle, ot, qs, k, W, rule, sent):
    if rule == 2:
        return oracle.ivfadc_batch_search(ot, qs, k)
    return oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule, n_threads=4)


IVF_CASES = ((5, 3, 0, 1000.0), (10, 2, 1, 100.0), (5, 1, 2, 100.0))


def _ivf_poisoned_batches(oracle, idx, ot, qs, m, what, need=(), forbid=(), cases=IVF_CASES, placements=util.PLACEMENTS):
    """Every placement x case: the oracle's lists for the poisoned batch, and the healthy queries' lists unchanged."""
    seen = set()
    for pi, placement in enumerate(placements):
        bad, mask = util.poison_batch(qs, placement, m, seed=pi)
        for k, W, rule, sent in cases:
            got, names = _profiled(idx, lambda: idx.search(bad, k, W, sentinel=sent, found_rule=rule))
            seen |= names
            w = f"{what} {placement} k={k} W={W} rule={rule}"
            util.assert_same_lists(got[0], got[1], _ivf_expect(oracle, ot, bad, k, W, rule, sent), w)
            ref = idx.search(qs, k, W, sentinel=sent, found_rule=rule)
            util.assert_rows_bit_equal(got, ref, ~mask, w)
            assert idx.bound_violations() == 0, w
    assert set(need) <= seen and not set(forbid) & seen, (what, sorted(seen))
    print(f"{what}: kernels {sorted(seen)}")
    return seen


def _rows_checked_are_the_healthy_queries(idx, qs, m, what):
    """check_brackets 1 (refine.h:520 counts every row that reaches the exact stage, whatever its distance): a poisoned query
    selects no cell and adds no row, a healthy one adds the rows of its W cells -- the batch with poisoned queries checks exactly
    as many rows as its healthy queries alone, fewer than the all-healthy batch."""
    k, W, rule, sent = IVF_CASES[0]
    bad, mask = util.poison_batch(qs, "every8", m)
    counts = []
    for batch in (bad, qs[~mask], qs):
        c0 = idx.bound_checked()
        idx.search(batch, k, W, sentinel=sent, found_rule=rule)
        counts.append(idx.bound_checked() - c0)
    print(f"{what}: rows checked {counts} (poisoned batch, its healthy queries alone, all healthy)")
    assert counts[0] == counts[1] and 0 < counts[1] < counts[2], (what, counts)
    assert idx.bound_violations() == 0, what


def _ivf(gpu, oracle, t):
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    return ot, gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])


def _qs(N=20000, n=Q, seed=7):
    return util.queries_from_corpus(N, n, seed=seed)[1]


# ---------------------------------------------------------------------------------------
# 1. poisoned queries, path by path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1024, 256])
def test_queries_filter_refine_scan(gpu, oracle, K, monkeypatch):
    """ivf_filter + merge_refine (K = 1024: slabs from HBM; K = 256: the LDS-resident variant), normally and with every
    probed row through the exact stage (check_brackets 1)."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t = util.ivf_tables(N=20000, C=32, K=K)
    ot, idx = _ivf(gpu, oracle, t)
    idx.set_option("sparse_items", 0)
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"filter + refine K={K}", need=("ivf_filter", "merge_refine"), forbid=("ivf_one", "adc_scan"))
    idx.set_option("check_brackets", 1)
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"filter + refine, every row, K={K}", need=("ivf_filter", "merge_refine"),
                          cases=IVF_CASES[:1], placements=("every8",))
    _rows_checked_are_the_healthy_queries(idx, _qs(), 12, f"filter + refine K={K}")
    idx.close()


@pytest.mark.parametrize("variant", ["3", "0"])
def test_queries_cell_major_fused_scan(gpu, oracle, variant, monkeypatch):
    """FREDDY_GPU_FUSED 1 with fused_kernel 3 (the reference's arithmetic for every row, cell-grouped) and FREDDY_GPU_FUSED 0
    (lut_build + adc_scan + merge_replay)."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1" if variant == "3" else "0")
    if variant == "3":
        monkeypatch.setenv("FREDDY_GPU_FUSED_KERNEL", "3")
    ot, idx = _ivf(gpu, oracle, util.ivf_tables(N=20000, C=32, K=256))
    need = ("ivf_exact_scan",) if variant == "3" else ("lut_build", "adc_scan")
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"fused variant {variant}", need=need, forbid=("ivf_filter",))
    idx.close()


@pytest.mark.parametrize("K", [256, 1024])
def test_queries_item_wise_sparse_scan(gpu, oracle, K, monkeypatch):
    """sparse_items -16: every cell item by item (two queries share a cell's rows in the pair units), also with every row refined."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    ot, idx = _ivf(gpu, oracle, util.ivf_tables(N=20000, C=32, K=K))
    idx.set_option("sparse_items", -16)
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"item-wise scan K={K}", need=("sparse_items", "merge_refine"))
    idx.set_option("check_brackets", 1)
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"item-wise scan, every row, K={K}", need=("sparse_items",), cases=IVF_CASES[:1],
                          placements=("every8",))
    _rows_checked_are_the_healthy_queries(idx, _qs(), 12, f"item-wise scan K={K}")
    idx.close()


def test_queries_cell_grouped_exact_scan_other_shape(gpu, oracle):
    """(d, m, K, C) = (25, 5, 256, 32): ivf_multi_scan (eight queries per cell) when forced, lut_build + adc_scan when off."""
    N = 8000
    ot, idx = _ivf(gpu, oracle, util.shape_ivf_tables(25, 5, 256, 32, N))
    qs = util.shape_queries(N, 25, Q, seed=3)
    idx.set_option("fused", 1)
    _ivf_poisoned_batches(oracle, idx, ot, qs, 5, "multi scan (25, 5, 256, 32)", need=("ivf_multi_scan",), forbid=("ivf_filter",))
    idx.set_option("fused", 0)
    _ivf_poisoned_batches(oracle, idx, ot, qs, 5, "generic scan (25, 5, 256, 32)", need=("adc_scan",), forbid=("ivf_multi_scan",),
                          placements=("every8",))
    idx.close()


@pytest.mark.parametrize("mode", ["normal", "refine_all", "off"])
def test_queries_mfma_cell_selection(gpu, oracle, mode, monkeypatch):
    """coarse_table + probe_plan (MFMA coarse tiles shared by 64 queries), with every cell refined, and the all-exact kernel."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    ot, idx = _ivf(gpu, oracle, util.ivf_tables(N=20000, C=32, K=256))
    idx.set_option("coarse_approx", 0 if mode == "off" else 1)
    if mode == "refine_all":
        idx.set_option("check_brackets", 2)
    cases = ((5, 3, 0, 1000.0), (3, 1, 1, 100.0), (8, 10, 0, 1000.0))
    need = ("coarse_dist",) if mode == "off" else ("coarse_table", "probe_plan")
    c0 = idx.coarse_bound_checked()
    _ivf_poisoned_batches(oracle, idx, ot, _qs(), 12, f"cell selection {mode}", need=need, cases=cases)
    if mode == "refine_all":
        # coarse.h:688: every query adds its n_all cells, a poisoned one too (:665 only skips the comparison when eps is not
        # finite or the MFMA value is a NaN): two calls per case and placement, all 32 cells of all Q queries in round one
        assert idx.coarse_bound_checked() - c0 >= 2 * len(cases) * len(util.PLACEMENTS) * Q * 32
    idx.close()


def test_queries_mfma_cell_selection_beyond_1024_cells(gpu, oracle, monkeypatch):
    """C = 1500: the streamed plan (tile minima, candidates as a bitmap), normally and with every cell refined."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    from freddy_amd import index_build as ib
    N, C = 30000, 1500
    t = ib.build_ivf_index(util.corpus(N), C=C, m=12, K=256, train_size=8000, iters=3, seed=4)
    ot, idx = _ivf(gpu, oracle, t)
    qs = _qs(N, Q, seed=3)
    idx.set_option("coarse_approx", 1)
    cases = ((5, 10, 0, 1000.0), (10, 1, 1, 100.0))
    _ivf_poisoned_batches(oracle, idx, ot, qs, 12, "1500 cells", need=("coarse_table", "probe_plan"), cases=cases, placements=("every8", "run64"))
    idx.set_option("check_brackets", 2)
    _ivf_poisoned_batches(oracle, idx, ot, qs, 12, "1500 cells, every cell", need=("coarse_table",), cases=cases[:1], placements=("ends",))
    idx.close()


def _alternate(search, expect, qs, bad, what):
    """Poisoned and healthy single queries in turn on one handle: every call's words meet the previous call's."""
    order = []
    for i in range(8):
        order += [("bad", i % len(bad)), ("good", i)]
    out = []
    for kind, i in order:
        q = bad[i] if kind == "bad" else qs[i]
        gi, gd = search(q[None])
        util.assert_same_lists(gi, gd, expect(q)[None], f"{what}: call {len(out)} ({kind} {i})")
        out.append((gi, gd))
    return out


def _single_poisons(qs, m):
    rng = np.random.default_rng(5)
    return [util.poison_query(qs[20 + j], kind, m, rng, "first" if j % 2 else "last") for j, kind in enumerate(util.QUERY_POISONS)]


@pytest.mark.parametrize("K", [256, 1024])
def test_queries_pq_one_launch(gpu, oracle, K):
    """pq_one: the table words published from NaNs carry the epoch like any other; 16 alternating calls, then the same calls
    with one_launch = 0 give the same bits."""
    N = 20000
    t = util.pq_tables(N=N, K=K)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    qs = _qs(N, 40, seed=5)
    bad = _single_poisons(qs, 12)
    _, names = _profiled(idx, lambda: idx.search(bad[0][None], 5, sentinel=100.0))
    assert "pq_one" in names, sorted(names)
    one = _alternate(lambda q: idx.search(q, 5, sentinel=100.0), lambda q: oracle.pq_search(ot, q, 5), qs, bad, f"pq_one K={K}")
    idx.set_option("one_launch", 0)
    _, names = _profiled(idx, lambda: idx.search(bad[0][None], 5, sentinel=100.0))
    assert "pq_one" not in names, sorted(names)
    three = _alternate(lambda q: idx.search(q, 5, sentinel=100.0), lambda q: oracle.pq_search(ot, q, 5), qs, bad, f"three launches K={K}")
    for a, b in zip(one, three):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    idx.close()


@pytest.mark.parametrize("K", [256, 1024])
def test_queries_ivf_one_launch(gpu, oracle, K):
    """ivf_one: coarse distances, cell list and tables of a poisoned query, alternating with healthy ones; one_launch = 0 as the cross-check."""
    N = 20000
    ot, idx = _ivf(gpu, oracle, util.ivf_tables(N=N, C=32, K=K))
    qs = _qs(N, 40, seed=17)
    bad = _single_poisons(qs, 12)
    _, names = _profiled(idx, lambda: idx.search(qs[:1], 5, 4, sentinel=1000.0, found_rule=0))
    assert "ivf_one" in names, sorted(names)
    for k, W, rule, sent in ((5, 4, 0, 1000.0), (10, 2, 1, 100.0)):
        idx.set_option("one_launch", 1)
        one = _alternate(lambda q: idx.search(q, k, W, sentinel=sent, found_rule=rule),
                         lambda q: oracle.ivfadc_search(ot, q, k, W, sentinel=sent, found_rule=rule), qs, bad, f"ivf_one K={K} rule={rule}")
        idx.set_option("one_launch", 0)
        multi = _alternate(lambda q: idx.search(q, k, W, sentinel=sent, found_rule=rule),
                           lambda q: oracle.ivfadc_search(ot, q, k, W, sentinel=sent, found_rule=rule), qs, bad, f"multi-launch K={K} rule={rule}")
        for a, b in zip(one, multi):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert idx.bound_violations() == 0
    idx.close()


def test_queries_k_beyond_512(gpu, oracle):
    """k = 600: merge_select + bigk_replay, IVFADC and flat PQ."""
    N = 20000
    ot, idx = _ivf(gpu, oracle, util.ivf_tables(N=N, C=32, K=256))
    qs = _qs(N, Q)
    _ivf_poisoned_batches(oracle, idx, ot, qs, 12, "k = 600", need=("merge_select", "bigk_replay"), cases=((600, 2, 0, 1000.0), (600, 1, 1, 100.0)),
                          placements=("every8",))
    idx.close()
    t = util.pq_tables(N=N, K=256)
    pt = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    pidx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    bad, mask = util.poison_batch(qs[:24], "every8", 12)
    got, names = _profiled(pidx, lambda: pidx.search(bad, 600, sentinel=100.0))
    assert "bigk_replay" in names, sorted(names)
    util.assert_same_lists(got[0], got[1], np.stack([oracle.pq_search(pt, q, 600) for q in bad]), "pq k = 600")
    util.assert_rows_bit_equal(got, pidx.search(qs[:24], 600, sentinel=100.0), ~mask, "pq k = 600")
    pidx.close()


@pytest.mark.parametrize("K", [256, 1024])
def test_queries_pq_batch_and_subset(gpu, oracle, K):
    """pq_search batches through pq_front (the cell-grouped scan) and the generic kernels, and the subset form."""
    N = 20000
    t = util.pq_tables(N=N, K=K)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    qs = _qs(N, Q)
    rng = np.random.default_rng(3)
    targets = np.concatenate([rng.choice(np.arange(1, N + 1), size=3000, replace=False), [N + 5, -3]]).astype(np.int32)
    for mode in (1, 0):
        idx.set_option("pq_fused", mode)
        for pi, placement in enumerate(util.PLACEMENTS):
            bad, mask = util.poison_batch(qs, placement, 12, seed=pi)
            got, names = _profiled(idx, lambda: idx.search(bad, 5, sentinel=100.0))
            w = f"pq batch K={K} pq_fused={mode} {placement}"
            assert ("pq_front" in names) == (mode == 1), (w, sorted(names))
            util.assert_same_lists(got[0], got[1], np.stack([oracle.pq_search(ot, q, 5) for q in bad]), w)
            util.assert_rows_bit_equal(got, idx.search(qs, 5, sentinel=100.0), ~mask, w)
            got = idx.search(bad, 7, sentinel=1000.0, subset_ids=targets)
            util.assert_same_lists(got[0], got[1], oracle.pq_search_in_batch(ot, bad, 7, targets), w + " subset")
            util.assert_rows_bit_equal(got, idx.search(qs, 7, sentinel=1000.0, subset_ids=targets), ~mask, w + " subset")
            assert idx.bound_violations() == 0, w
    idx.close()


def test_grouping_nonfinite_group_vectors(gpu, oracle):
    """grouping_pq: a poisoned group vector is never the nearest (its distances are NaN or Inf, never < 100); with only
    poisoned groups every row gets group -1."""
    N = 6000
    for d, m, K in ((300, 12, 256), (55, 11, 16)):
        t = util.shape_pq_tables(d, m, K, N)
        ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
        idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
        gv, mask = util.poison_batch(np.tile(util.shape_queries(N, d, 17), (8, 1)), "every8", m)
        for g in (gv[:37], gv[mask][:6]):
            gi, gg = idx.grouping(g)
            ei, eg = oracle.grouping_pq(ot, g, t["ids"])
            assert np.array_equal(gi, ei) and np.array_equal(gg, eg), (d, m, K, len(g))
        assert (gg == -1).all()
        idx.close()


def test_encode_insert_kmeans_nonfinite_vectors(gpu, oracle):
    """encode, insert_quantize and kmeans with NaN and Inf vectors among the rows: the strict-< argmins of the oracle."""
    N, d, m, K = 3000, 300, 12, 256
    x = util.shape_corpus(N, d).numpy()
    rng = np.random.default_rng(8)
    cb = (rng.standard_normal((m, K, d // m)) * 0.05).astype(np.float32)
    vecs, mask = util.poison_batch(x[:Q], "every8", m)
    coarse = x[rng.choice(N, 65, replace=False)].copy()
    cell, codes = gpu.encode(cb, vecs, coarse=coarse)
    exp_cell = oracle.assign_coarse(coarse, vecs)
    assert np.array_equal(cell, exp_cell)
    res = np.stack([oracle.vec_minus(vecs[i], coarse[exp_cell[i]]) for i in range(len(vecs))])
    assert np.array_equal(codes, oracle.encode_pq(cb, res))
    assert np.array_equal(gpu.encode(cb, vecs)[1], oracle.encode_pq(cb, vecs))
    # insert_quantize starts every argmin from 100 (1000 for the multi-index): the oracle refuses a vector with no code
    # (the reference would use an uninitialised one); the healthy rows of the same batch quantise as they do alone
    out = gpu.insert_quantize(vecs[~mask], pq_codebook=cb)
    cb2, _, ecodes, _ = oracle.update_codebook(cb, np.ones(m * K, np.int32), vecs[~mask])
    assert np.array_equal(out["pq_codes"], ecodes)
    for v in vecs[mask][:6]:     # one of each poison: no codeword is nearer than 100, which the oracle and the library both refuse
        with pytest.raises(ValueError):
            oracle.update_codebook(cb, np.ones(m * K, np.int32), v[None])
        with pytest.raises(gpu.FreddyGpuError, match="100 or farther"):
            gpu.insert_quantize(v[None], pq_codebook=cb)
    train = np.concatenate([x[200:500], vecs[mask][:2]])
    init = rng.choice(300, 7, replace=False).astype(np.int32)
    gc, ga = gpu.kmeans(train, 7, 3, init)
    oc, oa = oracle.kmeans(train, 7, 3, init)
    assert np.array_equal(ga, oa)
    nan_g, nan_o = np.isnan(gc), np.isnan(oc)
    assert np.array_equal(nan_g, nan_o) and nan_o.any()
    assert np.array_equal(gc.view(np.uint32)[~nan_o], oc.view(np.uint32)[~nan_o])


# ---------------------------------------------------------------------------------------
# 2. poisoned tables: pinned, and brought in by update_codebook / append_rows
# ---------------------------------------------------------------------------------------
def _busy_code(t, pos):
    return int(np.argmax(np.bincount(t["codes"][:, pos].astype(np.int64), minlength=t["codebook"].shape[1])))


UNUSED_POS = 11


def _free_last_code(t):
    """t with code K - 1 of position 11 given up by its rows (they take code 0): a codeword that no row uses."""
    codes = t["codes"].copy()
    codes[codes[:, UNUSED_POS] == t["codebook"].shape[1] - 1, UNUSED_POS] = 0
    return dict(t, codes=codes)


def _poisoned_ivf_table(t, kind, qs):
    """(coarse, codebook) with the table poison `kind`; t from _free_last_code."""
    coarse, cb = t["coarse"].copy(), t["codebook"].copy()
    K = cb.shape[1]
    near = np.bincount(np.argmin(((qs[:, None, :] - coarse[None]) ** 2).sum(-1), axis=1), minlength=coarse.shape[0])
    cell = int(np.argmax(near))                     # some queries' nearest cell; not empty
    assert near[cell] > 0 and t["list_off"][cell + 1] > t["list_off"][cell]
    if kind == "centroid_nan":
        coarse[cell, 17] = np.nan
    elif kind == "centroid_inf":
        coarse[cell, 299] = np.inf
    elif kind == "codeword_nan":
        used = _busy_code(t, 0)
        assert (t["codes"][:, 0] == used).sum() >= 100
        cb[0, used, 3] = np.nan
        assert not (t["codes"][:, UNUSED_POS] == K - 1).any()
        cb[UNUSED_POS, K - 1, 0] = np.nan             # ... and one that no row uses
    elif kind == "codeword_inf":
        cb[5, _busy_code(t, 5), 24] = np.inf
    elif kind == "slice_nan":
        cb[11] = np.nan
    return coarse, cb


@pytest.mark.parametrize("kind", ["centroid_nan", "centroid_inf", "codeword_nan", "codeword_inf", "slice_nan"])
@pytest.mark.parametrize("K", [256, 1024])
def test_tables_ivfadc(gpu, oracle, kind, K, monkeypatch):
    """A poisoned centroid or codeword in a handle of its own, through the filter + refine scan (normally and with every row
    and every cell refined), the item-wise scan, the generic kernels and the one-launch kernel; the codebook poisons also
    brought in by update_codebook on a healthy handle: the same lists as the fresh pin."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    t = _free_last_code(util.ivf_tables(N=20000, C=32, K=K))
    qs = _qs(20000, 70)
    coarse, cb = _poisoned_ivf_table(t, kind, qs)
    ot = oracle.ivf_table(coarse, cb, t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(coarse, cb, t["list_off"], t["ids"], t["codes"])
    cases = ((5, 3, 0, 1000.0), (10, 2, 1, 100.0), (5, 1, 2, 100.0))
    exp = [_ivf_expect(oracle, ot, qs, *c) for c in cases]
    fresh = []

    def run(ix, what, keep=None):
        for c, e in zip(cases, exp):
            k, W, rule, sent = c
            gi, gd = ix.search(qs, k, W, sentinel=sent, found_rule=rule)
            util.assert_same_lists(gi, gd, e, f"{kind} K={K} {what} k={k} W={W} rule={rule}")
            if keep is not None:
                keep.append((gi, gd))
        assert ix.bound_violations() == 0, (kind, K, what)

    run(idx, "filter + refine", fresh)
    idx.set_option("check_brackets", 3)
    rows0, cells0 = idx.bound_checked(), idx.coarse_bound_checked()
    run(idx, "every row and every cell refined")
    rows1, cells1 = idx.bound_checked() - rows0, idx.coarse_bound_checked() - cells0
    idx.set_option("check_brackets", 0)
    # every cell of every query is checked in round one whatever its centroid holds (coarse.h:688 counts n_all; :665 only skips
    # the comparison), and a codebook poison changes no cell choice: the rows checked are those of the healthy table
    assert cells1 >= len(cases) * len(qs) * 32, (kind, K, cells1)
    if not kind.startswith("centroid"):
        href = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
        href.set_option("check_brackets", 3)
        for k, W, rule, sent in cases[:1]:
            href.search(qs, k, W, sentinel=sent, found_rule=rule)
        h_rows = href.bound_checked()
        href.close()
        idx.set_option("check_brackets", 3)
        r0 = idx.bound_checked()
        idx.search(qs, *cases[0][:2], sentinel=cases[0][3], found_rule=cases[0][2])
        print(f"{kind} K={K}: rows checked {idx.bound_checked() - r0}, healthy table {h_rows}")
        assert idx.bound_checked() - r0 == h_rows > 0, (kind, K)
        idx.set_option("check_brackets", 0)
    assert rows1 > 0
    idx.set_option("sparse_items", -16)
    run(idx, "item-wise scan")
    idx.set_option("sparse_items", 0)
    idx.set_option("coarse_approx", 0)
    run(idx, "all-exact cell selection")
    idx.set_option("coarse_approx", 1)
    idx.set_option("fused", 0)
    run(idx, "generic kernels")
    idx.set_option("fused", -1)
    for i in range(12):     # single queries through ivf_one and, as the cross-check, the multi-launch path
        for one in (1, 0):
            idx.set_option("one_launch", one)
            gi, gd = idx.search(qs[i][None], 5, 3, sentinel=1000.0, found_rule=0)
            util.assert_same_lists(gi, gd, exp[0][i][None], f"{kind} K={K} single query {i} one_launch={one}")
    idx.close()
    if kind.startswith("codeword") or kind == "slice_nan":
        idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
        idx.search(qs, 5, 3, sentinel=1000.0, found_rule=0)
        idx.update_codebook(cb)
        swapped = []
        run(idx, "after update_codebook", swapped)
        for a, b in zip(fresh, swapped):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        idx.close()


@pytest.mark.parametrize("K", [256, 1024])
def test_tables_pq(gpu, oracle, K):
    """Flat PQ with a NaN codeword that 100+ rows use and one no row uses, an Inf codeword, a whole NaN slice: pinned and by
    update_codebook; batches (pq_front, generic), single queries (pq_one), a subset, grouping_pq."""
    N = 20000
    t = _free_last_code(util.pq_tables(N=N, K=K))
    qs = _qs(N, 70)
    healthy = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    rng = np.random.default_rng(3)
    targets = rng.choice(np.arange(1, N + 1), size=3000, replace=False).astype(np.int32)
    for kind in ("codeword_nan", "codeword_inf", "slice_nan"):
        _, cb = _poisoned_ivf_table(dict(t, coarse=qs[:4], list_off=np.array([0, N // 4, N // 2, 3 * N // 4, N])), kind, qs)
        ot = oracle.pq_table(cb, t["ids"], t["codes"])
        exp = np.stack([oracle.pq_search(ot, q, 5) for q in qs])
        exp_sub = oracle.pq_search_in_batch(ot, qs, 5, targets)
        eg = oracle.grouping_pq(ot, qs[:9], t["ids"])
        fresh = gpu.PQIndex(cb, t["ids"], t["codes"])
        healthy.update_codebook(cb)
        for ix, what in ((fresh, "pinned"), (healthy, "update_codebook")):
            for mode in (1, 0):
                ix.set_option("pq_fused", mode)
                gi, gd = ix.search(qs, 5, sentinel=100.0)
                util.assert_same_lists(gi, gd, exp, f"pq {kind} K={K} {what} pq_fused={mode}")
                gi, gd = ix.search(qs, 5, sentinel=1000.0, subset_ids=targets)
                util.assert_same_lists(gi, gd, exp_sub, f"pq subset {kind} K={K} {what} pq_fused={mode}")
            for i in range(12):
                gi, gd = ix.search(qs[i][None], 5, sentinel=100.0)
                util.assert_same_lists(gi, gd, exp[i][None], f"pq_one {kind} K={K} {what} query {i}")
            gi, gg = ix.grouping(qs[:9])
            assert np.array_equal(gi, eg[0]) and np.array_equal(gg, eg[1]), (kind, K, what)
            assert ix.bound_violations() == 0
        fresh.close()
    healthy.close()


# ---------------------------------------------------------------------------------------
# 3. vector handles: a NaN row, an Inf row, a row whose norm overflows
# ---------------------------------------------------------------------------------------
def _nan_as_one(a):
    """similarity bits with every NaN as 0x7fc00000: which NaN an invalid operation produces is the processor's choice
    (0xffc00000 on x86, 0x7fc00000 on gfx950), not the arithmetic's."""
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _exact_same(gi, gs, exp, k, what):
    for qi, e in enumerate(exp):
        e = e[:k]
        n = len(e)
        assert gi[qi, :n].tolist() == e["id"].tolist(), (what, qi)
        assert np.array_equal(_nan_as_one(gs[qi, :n]), _nan_as_one(e["dist"])), (what, qi)
        assert (gi[qi, n:] == -1).all() and np.isneginf(gs[qi, n:]).all(), (what, qi)


def _vector_table(N=8192 + 40, d=64):
    x = util.shape_corpus(N, d).numpy().copy()
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    bad = {"nan": 700, "inf": 4100, "norm": 6000}
    rows = {"nan": x[700].copy(), "inf": x[4100].copy(), "norm": (x[6000] * np.float32(3e19)).astype(np.float32)}
    rows["nan"][5] = np.nan
    rows["inf"][d - 1] = np.inf
    qs = x[::N // 70][:70].copy()
    return x, ids, bad, rows, qs


@pytest.mark.parametrize("kind", ["nan", "inf", "norm"])
def test_vector_rows_exact_knn_and_join(gpu, oracle, kind):
    """The exact kNN (filter + refine where it is eligible, the all-exact scan, every row refined) and the exact join with the
    row inside and outside the target set; the row pinned with the table, and appended to a healthy handle."""
    x, ids, bad, rows, qs = _vector_table()
    r = bad[kind]
    xp = x.copy(); xp[r] = rows[kind]
    N = x.shape[0]
    # appended: the poisoned row comes last (ids ascend), the table is otherwise the healthy one
    xa = np.concatenate([x, rows[kind][None]]); ida = np.concatenate([ids, [ids[-1] + 2]]).astype(np.int32)
    rng = np.random.default_rng(4)
    inside = np.concatenate([ids[rng.choice(N, 2000, replace=False)], [ids[r]]]).astype(np.int32)
    outside = inside[inside != ids[r]]
    for what, tx, tid, make in (("pinned", xp, ids, lambda: gpu.VectorIndex(ids, xp)), ("appended", xa, ida, None)):
        if make is None:
            idx = gpu.VectorIndex(ids, x)
            idx.search(qs[:9], 5)
            idx.append_rows(ida[-1:], vectors=xa[-1:])
        else:
            idx = make()
        exp = [oracle.exact_knn(tx, tid, q, 32) for q in qs]
        for mode in (-1, 1, 0):
            idx.set_option("exact_filter", mode)
            for Qn, k in ((70, 5), (9, 32), (1, 1)):
                gi, gs = idx.search(qs[:Qn], k)
                _exact_same(gi, gs, exp[:Qn], k, f"exact kNN {kind} {what} exact_filter={mode} Q={Qn} k={k}")
        idx.set_option("exact_filter", -1)
        idx.set_option("check_brackets", 4)
        gi, gs = idx.search(qs, 5)
        _exact_same(gi, gs, exp, 5, f"exact kNN {kind} {what} every row refined")
        idx.set_option("check_brackets", 0)
        assert idx.bound_violations() == 0, (kind, what)
        for tg, tw in ((inside, "inside"), (outside, "outside")):
            if what == "appended":
                tg = np.concatenate([outside, ida[-1:]]) if tw == "inside" else outside
            gi, gs = idx.join(qs, 5, tg)
            _exact_same(gi, gs, [oracle.exact_knn(tx, tid, q, 5, tg) for q in qs], 5, f"exact join {kind} {what} row {tw}")
        assert idx.bound_violations() == 0, (kind, what, "join")
        idx.close()


# ---------------------------------------------------------------------------------------
# 4. the approximate kNN-join
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [0, 1])
def test_queries_knn_join(gpu, oracle, host):
    """ivpq_search_in with poisoned queries, methods 0 / 1 / 2, device and host traversal: a query whose cell keys are NaN or
    Inf ties on every key, so the device hands it to the host heap, which is the oracle's literal heap."""
    N = 20000
    t = util.ivpq_tables(N=N, m=30, K=32, k_coarse=8)
    ot = oracle.ivpq_table(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])
    idx = gpu.IVPQIndex(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])
    idx.set_option("join_host_traversal", host)
    qs = _qs(N, Q, seed=21)
    rng = np.random.default_rng(5)
    targets = rng.choice(np.arange(1, N + 1), size=4000, replace=False).astype(np.int32)
    compared = {0: 0, 1: 0, 2: 0}
    for pi, placement in enumerate(util.PLACEMENTS):
        bad, mask = util.poison_batch(qs, placement, 30, seed=pi)
        for method in (0, 1, 2):
            for tl in (True, False):
                gi, gd, git = idx.knn_join(bad, 5, targets, 3, 20, method, use_target_lists=tl, confidence=0.8)
                exp, eit = oracle.ivpq_search_in(ot, bad, 5, targets, 3, 20, method, use_target_lists=tl, confidence=0.8)
                w = f"join host={host} {placement} method={method} tl={tl}"
                assert git == eit, (w, git, eit)
                util.assert_same_lists(gi, gd, exp, w)
                hi, hd, hit = idx.knn_join(qs, 5, targets, 3, 20, method, use_target_lists=tl, confidence=0.8)
                # A poisoned query accepts no row and stays active until the batch's last round; a healthy query that the
                # all-healthy call retires in its only round is retired in round one here too and never touched again.
                if hit == 1:
                    util.assert_rows_bit_equal((gi, gd), (hi, hd), ~mask, w)
                    compared[method] += 1
    assert all(n >= len(util.PLACEMENTS) for n in compared.values()), compared
    idx.close()


# ---------------------------------------------------------------------------------------
# 5. post verification, analogies, appended rows, the batch UDF's cell limit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "inf", "norm"])
def test_vector_rows_search_pv(gpu, oracle, kind):
    """search_pv (IVFADC and flat PQ) with the poisoned raw row among a query's candidates: the row pinned with the vector
    table, and appended to a vector handle that lacked it.  Expected from the oracle alone (pv_model): a NaN similarity leads
    its query's list, the other queries' lists are those of the healthy table."""
    import pv_model as pm
    x, ids, qs, ivf, pq = pm.main_tables()
    qs = qs[:70]
    k, pvf, W = 5, 6, 3
    ivf_t = oracle.ivf_table(ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    pq_t = oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"])
    lists = {"ivf": pm.ivf_lists(oracle, ivf_t, qs, k * pvf, W), "pq": pm.pq_lists(oracle, pq_t, qs, k * pvf)}
    # the poisoned row: a candidate of the same query in both searches (ids are 1 .. N in row order)
    qi, rid = next((q, int(c[0])) for q in range(20, 70) for c in [np.intersect1d(lists["ivf"][q], lists["pq"][q])] if c.size and c[0] > 0)
    r = rid - 1
    assert ids[r] == rid and all(rid in lists[name][qi] for name in lists)
    xp = x.copy()
    if kind == "nan":
        xp[r, 5] = np.nan
    elif kind == "inf":
        xp[r, 299] = np.inf
    else:
        xp[r] = (x[r] * np.float32(3e19)).astype(np.float32)
    hi = gpu.IVFIndex(ivf["coarse"], ivf["codebook"], ivf["list_off"], ivf["ids"], ivf["codes"])
    hp = gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"])
    pinned = gpu.VectorIndex(ids, xp)
    appended = gpu.VectorIndex(ids[:r], x[:r])         # the rows below the poisoned one; it and the rest arrive by append_rows
    appended.search(qs[:3], 5)
    appended.append_rows(ids[r:], vectors=xp[r:])
    for vec, what in ((pinned, "pinned"), (appended, "appended")):
        for name, call in (("ivf", lambda: hi.search_pv(vec, qs, k, pvf, W)), ("pq", lambda: hp.search_pv(vec, qs, k, pvf))):
            exp, n_cand, n_scored = pm.expected(oracle, lists[name], xp, ids, qs, k)
            (gi, gs), names = _profiled(hi if name == "ivf" else hp, call)
            assert "pv_rerank" in names, sorted(names)
            _exact_same(gi, gs, exp, k, f"search_pv {name} {kind} {what}")
            st = (hi if name == "ivf" else hp).last_pv_stats()
            assert st == {"candidates": int(n_cand.sum()), "scored": int(n_scored.sum())}, (name, kind, what)
            if kind == "nan":
                assert gi[qi, 0] == rid and np.isnan(gs[qi, 0]), (name, kind, what)
    for h in (hi, hp, pinned, appended):
        h.close()


@pytest.mark.parametrize("kind", ["nan", "inf", "norm"])
def test_vector_rows_analogies(gpu, kind):
    """3CosAdd, 3CosMul and pair direction over a table with one non-finite row, against analogy_model / pair_model: the row as
    a candidate of every analogy and as each of the three inputs.  analogy.h says such tables need no other path -- there is
    no filter pass for them (a NaN or Inf element; the finite overflowing row keeps the filter), the arithmetic just runs."""
    import analogy_model as am
    import pair_model as pr
    N, d = 8192 + 40, 300
    x = util.corpus(N).numpy().copy()
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    r = 4100
    if kind == "nan":
        x[r, 7] = np.nan
    elif kind == "inf":
        x[r, d - 1] = np.inf
    else:
        x[r] = (x[r] * np.float32(3e19)).astype(np.float32)
    rng = np.random.default_rng(6)
    t = rng.integers(0, N, size=(11, 3))
    t[1], t[2], t[3] = (r, 17, 900), (33, r, 901), (44, 55, r)
    t[4] = (r - 1, r + 1, r - 2)                       # neighbours in the same block
    triples = ids[t]
    x_t = np.ascontiguousarray(x.T)
    idx = gpu.VectorIndex(ids, x)
    with np.errstate(all="ignore"):
        for method in ("3cosadd", "3cosmul", "pair_direction"):
            ei, es = (pr.model(x, ids, triples, 5, x_t=x_t) if method == "pair_direction" else am.model(x, ids, triples, 5, method, x_t=x_t))
            for mode in (-1, 0):
                idx.set_option("exact_filter", mode)
                gi, gs = idx.analogy(triples, k=5, method=method)
                bad = np.nonzero((gi != ei).any(1) | (gs.view(np.uint64) != es.view(np.uint64)).any(1))[0]
                assert bad.size == 0, (kind, method, mode, bad[:5], gi[bad[:1]], ei[bad[:1]], gs[bad[:1]], es[bad[:1]])
                st = idx.last_analogy_stats()
                if kind != "norm" or mode == 0 or method == "pair_direction":
                    assert st["filter_passes"] == 0, (kind, method, mode, st)
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("K", [256, 1024])
def test_tables_poison_met_by_appended_rows(gpu, oracle, K, monkeypatch):
    """A NaN and an Inf codeword that no pinned row uses, and a NaN centroid whose cell holds rows: append_rows then brings rows
    that use those codewords, some of them into that cell.  IVFADC and flat PQ, against the oracle over the model's tables
    (mutation_model) and against a fresh pin of them."""
    import mutation_model as mm
    monkeypatch.setenv("FREDDY_GPU_FUSED", "1")
    N, n_new = 20000, 400
    qs = _qs(N, 70)
    rng = np.random.default_rng(K)
    new_ids = np.arange(N + 1, N + 1 + n_new, dtype=np.int32)
    new_codes = rng.integers(0, K - 1, (n_new, 12)).astype(np.int16)
    new_codes[::3, UNUSED_POS] = K - 1                 # the NaN codeword
    new_codes[1::7, 0] = K - 1                         # the Inf codeword
    # IVFADC
    t = _free_last_code(util.ivf_tables(N=N, C=32, K=K))
    codes = t["codes"].copy()
    codes[codes[:, 0] == K - 1, 0] = 0
    coarse, cb = _poisoned_ivf_table(t, "centroid_nan", qs)
    cb[UNUSED_POS, K - 1, 0] = np.nan
    cb[0, K - 1, 24] = np.inf
    bad_cell = int(np.nonzero(np.isnan(coarse).any(1))[0][0])
    new_cell = rng.integers(0, 32, n_new).astype(np.int32)
    new_cell[::5] = bad_cell
    model = mm.IVFModel(coarse, cb, t["list_off"], t["ids"], codes)
    idx = gpu.IVFIndex(*model.pin_args())
    idx.search(qs, 5, 3, sentinel=1000.0, found_rule=0)
    model.append(new_ids, new_cell, new_codes)
    idx.append_rows(new_ids, coarse_id=new_cell, codes=new_codes)
    ot = model.oracle_table(oracle)
    fresh = gpu.IVFIndex(*model.pin_args())
    for sparse in (0, -16):
        for brackets in (0, 3):
            for ix in (idx, fresh):
                ix.set_option("sparse_items", sparse)
                ix.set_option("check_brackets", brackets)
            for k, W, rule, sent in IVF_CASES:
                a = idx.search(qs, k, W, sentinel=sent, found_rule=rule)
                b = fresh.search(qs, k, W, sentinel=sent, found_rule=rule)
                w = f"appended K={K} sparse_items={sparse} check_brackets={brackets} k={k} W={W} rule={rule}"
                util.assert_same_lists(a[0], a[1], _ivf_expect(oracle, ot, qs, k, W, rule, sent), w)
                util.assert_rows_bit_equal(a, b, slice(None), w)
    assert idx.bound_violations() == 0 and fresh.bound_violations() == 0
    idx.close(); fresh.close()
    # flat PQ
    p = _free_last_code(util.pq_tables(N=N, K=K))
    pcodes = p["codes"].copy()
    pcodes[pcodes[:, 0] == K - 1, 0] = 0
    pcb = p["codebook"].copy()
    pcb[UNUSED_POS, K - 1, 0] = np.nan
    pcb[0, K - 1, 24] = np.inf
    pmodel = mm.PQModel(pcb, p["ids"], pcodes)
    pidx = gpu.PQIndex(*pmodel.pin_args())
    pidx.search(qs, 5, sentinel=100.0)
    pmodel.append(new_ids, new_codes)
    pidx.append_rows(new_ids, codes=new_codes)
    pt = pmodel.oracle_table(oracle)
    pfresh = gpu.PQIndex(*pmodel.pin_args())
    exp = np.stack([oracle.pq_search(pt, q, 5) for q in qs])
    for mode in (1, 0):
        for ix, what in ((pidx, "appended"), (pfresh, "fresh pin")):
            ix.set_option("pq_fused", mode)
            gi, gd = ix.search(qs, 5, sentinel=100.0)
            util.assert_same_lists(gi, gd, exp, f"pq {what} K={K} pq_fused={mode}")
            gi, gd = ix.search(qs[:1], 5, sentinel=100.0)
            util.assert_same_lists(gi, gd, exp[:1], f"pq_one {what} K={K}")
    assert pidx.bound_violations() == 0
    pidx.close(); pfresh.close()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_queries_batch_udf_cell_limit(gpu, oracle, fused, monkeypatch):
    """Data x 14: every coarse distance lies in [100, 1000), where ivfadc_batch_search (argmin from 1000) keeps probing and
    ivfadc_search's cell list (sentinel 100) admits no cell -- with poisoned queries in the batch."""
    monkeypatch.setenv("FREDDY_GPU_FUSED", fused)
    scale = np.float32(14.0)
    t = dict(util.ivf_tables(N=20000, C=32, K=256))
    t["coarse"] = (t["coarse"] * scale).astype(np.float32)
    t["codebook"] = (t["codebook"] * scale).astype(np.float32)
    ot, idx = _ivf(gpu, oracle, t)
    qs = (_qs() * scale).astype(np.float32)
    qs[::2] += np.float32(0.04) * scale
    e2 = oracle.ivfadc_batch_search(ot, qs, 5)
    e1 = oracle.ivfadc_search_many(ot, qs, 5, 1, sentinel=100.0, found_rule=1)
    assert not np.array_equal(e2["id"], e1["id"]), "the two cell limits must be told apart by this test"
    _ivf_poisoned_batches(oracle, idx, ot, qs, 12, f"cell limit, FREDDY_GPU_FUSED={fused}", cases=((5, 1, 2, 100.0), (5, 1, 1, 100.0)))
    idx.close()
