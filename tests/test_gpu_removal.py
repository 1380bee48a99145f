"""-m gpu: freddy_gpu_remove_rows, the third way a pinned handle changes, in sequences that mix it with append_rows and
update_codebook on every handle kind.  tests/removal_model.py applies every step to host arrays; after every step the checks
of tests/test_gpu_mutation.py for that kind compare the handle with the CPU oracle on the model's tables (ids, ranks, distance
bits) and with a FRESH pin of them (ids and float bits, the kernel that served each call, bound_violations() == 0).  Nothing
here has a tolerance.

What is removed is chosen by the layouts' edges: lane 0 and lane 63 of a 64-row block, a whole middle block, a list going
65 -> 64 -> 63 rows, a whole cell (a second probing round), appended rows, every third row of a list of more than 256 blocks,
the row with the largest id (a later append may then start above the id that is left), a middle row and the ends of an ivpq
table (ids_affine), 32-row strips and 64-row blocks of a vector table, the row with the largest element, the only non-finite
row, every row.  removed counts, refusals, freddy_gpu_index_bytes and the host mirror's delete_rows follow."""
import numpy as np
import pytest

import removal_model as rm
import test_gpu_mutation as tm
import util

pytestmark = pytest.mark.gpu

E_ARG = tm.E_ARG
UNKNOWN = [10 ** 8 + 1, 10 ** 8 + 3]          # ids no table here has


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _remove(idx, model, ids, what):
    """the same ids (shuffled, some twice, some unknown) to the handle and to the model: equal counts, equal row counts"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    ask = np.concatenate([ids, ids[:3], UNKNOWN])
    ask = ask[np.random.default_rng(ask.size).permutation(ask.size)]
    got, exp = idx.remove_rows(ask), model.remove(ask)
    assert got == exp == np.unique(ids).size, (what, got, exp, np.unique(ids).size)
    assert idx.N == model.N, what
    return got


def _same_bytes(idx, fresh_cls, model, what, **kw):
    fresh = fresh_cls(*model.pin_args(), **kw)
    assert idx.nbytes == fresh.nbytes, (what, "freddy_gpu_index_bytes", idx.nbytes, fresh.nbytes)
    fresh.close()


# =======================================================================================
# 1. IVFADC
# =======================================================================================
def _ivf_rows(shape):
    """tm._ivf_source with the rows of the two largest cells first (pinned whole: lists of three blocks and more) and ids
    1..N in that order -> (coarse, codebook, ids, cell, codes, vectors, rows of the two cells)"""
    coarse, cb, ids, cell, codes, x = tm._ivf_source(*shape)
    big = np.argsort(-np.bincount(cell, minlength=shape[3]), kind="stable")[:2]
    first = np.isin(cell, big)
    order = np.concatenate([np.nonzero(first)[0], np.nonzero(~first)[0]])
    return coarse, cb, ids, cell[order], codes[order], np.ascontiguousarray(x[order]), int(first.sum())


IVF_CASES = [(300, 12, 256, 32), (300, 12, 1024, 32), (100, 5, 64, 16)]


@pytest.mark.parametrize("shape", IVF_CASES, ids=["300x12x256x32", "300x12x1024x32", "100x5x64x16"])
def test_ivf_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, shape):
    d, m, K, C = shape
    special = m == 12 and d == 300
    coarse, cb, ids, cell, codes, x, n_big = _ivf_rows(shape)
    n0 = n_big + 2600
    model = rm.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    idx = gpu.IVFIndex(*model.pin_args())
    by_len = [int(c) for c in np.argsort([-model.list_len(c) for c in range(C)], kind="stable")]
    A, B, D, E = by_len[0], by_len[1], by_len[2], by_len[3]
    assert model.list_len(A) >= 193 and model.list_len(B) >= 193 and model.list_len(D) >= 66, [model.list_len(c) for c in (A, B, D)]
    rng = np.random.default_rng(K + C)
    in_E = np.nonzero(cell[:n0] == E)[0]
    qrows = np.concatenate([rng.choice(n0, 30, replace=False), in_E[:3], [n0 + 3, n0 + 250]])
    qs = np.ascontiguousarray(x[qrows])
    assert (oracle.assign_coarse(coarse, qs) == E).any(), "no query probes the cell that will be emptied first"
    la, lb, ld = model.list_ids[A].copy(), model.list_ids[B].copy(), model.list_ids[D].copy()
    n1, n2 = n0 + 300, n0 + 500

    def check(what, full=True):
        _same_bytes(idx, gpu.IVFIndex, model, what)
        if full:
            tm._ivf_check(gpu, oracle, idx, model, qs, special, K <= 256, what)
        else:
            fresh = gpu.IVFIndex(*model.pin_args())
            got = idx.search(qs, 5, 3)
            util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3), what)
            tm._bits_equal(got, fresh.search(qs, 5, 3), what)
            fresh.close()

    # single rows and 64 rows of lists of three blocks and more (a fresh pin arranges a list's rows for the LDS banks, so these ids
    # sit in scattered lanes; the lanes of APPENDED rows are known: see below)
    _remove(idx, model, np.concatenate([la[:1], la[127:128], lb[64:128]]), "scattered lanes")
    check("ivf: rows out of lists of three blocks")
    # a list of 65, 64, 63 rows
    _remove(idx, model, ld[65:], "to 65"); assert model.list_len(D) == 65
    check("ivf: a list of 65 rows", full=False)
    _remove(idx, model, ld[10:11], "to 64"); assert model.list_len(D) == 64
    check("ivf: a list of 64 rows", full=False)
    _remove(idx, model, ld[64:65], "to 63"); assert model.list_len(D) == 63
    check("ivf: a list of 63 rows")
    # a whole cell: the queries nearest to it go into a second probing round
    _remove(idx, model, model.list_ids[E].copy(), "a cell")
    near = oracle.assign_coarse(coarse, qs)
    assert model.list_len(E) == 0 and sum(1 for c in near if model.list_len(int(c)) < 30) > 0
    check("ivf: an empty cell")
    cb2 = tm._nudged(model.codebook, 77)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    # appended rows leave again, the row with the largest id among them.  The first 70 go to list D behind its 63 rows: row 0 takes
    # lane 63 of block 0, rows 1..64 are block 1 (a middle block: rows 65..69 open block 2) -- removed: lane 63 of a block, then a
    # whole middle block with its lane 0
    sl = slice(n0, n1)
    to = cell[sl].copy(); to[:70] = D
    idx.append_rows(ids[sl], coarse_id=to, codes=codes[sl]); model.append(ids[sl], to, codes[sl])
    assert model.list_len(D) >= 63 + 70
    _remove(idx, model, ids[n0:n0 + 1], "lane 63 of a block")
    check("ivf: lane 63 of a block", full=False)
    _remove(idx, model, np.concatenate([ids[n0 + 1:n0 + 65], ids[n1 - 10:n1], la[1:30]]), "appended rows")
    assert model.max_id == int(ids[n1 - 11])
    check("ivf: appended rows removed, the largest id among them")
    # an id between the new and the old maximum is accepted, as on a fresh pin
    back = slice(n1 - 5, n2)
    idx.append_rows(ids[back], coarse_id=cell[back], codes=codes[back]); model.append(ids[back], cell[back], codes[back])
    check("ivf: an append above the largest id that was left")
    # refused: the answers and the footprint stay
    before, nbytes = [idx.search(qs, 5, 3), idx.search(qs[:1], 5, 3)], idx.nbytes
    bad = np.array([int(la[40]), int(la[41]), -3, int(la[42])], np.int32)
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*id -3 at position 2"):
        idx.remove_rows(bad)
    with pytest.raises(rm.Refused):
        model.remove(bad)
    gpu._check(idx.lib.freddy_gpu_remove_rows(idx.h, 0, None, None))
    assert idx.remove_rows(UNKNOWN) == 0 and idx.nbytes == nbytes and idx.N == model.N
    for a, b in zip(before, [idx.search(qs, 5, 3), idx.search(qs[:1], 5, 3)]):
        tm._bits_equal(a, b, "ivf: after the refused call")
    # every row
    _remove(idx, model, np.concatenate(model.list_ids), "every row")
    assert idx.N == 0 and model.max_id == -1
    check("ivf: empty", full=False)
    tail = slice(n2, n2 + 200)
    idx.append_rows(ids[10:11], coarse_id=cell[10:11], codes=codes[10:11]); model.append(ids[10:11], cell[10:11], codes[10:11])   # a small id: the handle is empty
    idx.append_rows(ids[tail], coarse_id=cell[tail], codes=codes[tail]); model.append(ids[tail], cell[tail], codes[tail])
    check("ivf: appended to the emptied handle")
    idx.close()


def test_ivf_a_list_of_more_than_256_blocks_thinned_by_every_third_row(gpu, oracle):
    """16 600 rows go into one cell (more than 256 blocks: rm_list_scan_kernel walks the list in several rounds with a carry),
    then every third row of that list leaves."""
    coarse, cb, ids, cell, codes, x = tm._ivf_source(300, 12, 256, 32)
    n0, X, grow = 3000, 5, 16600
    model = rm.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    idx = gpu.IVFIndex(*model.pin_args())
    sl = slice(n0, n0 + grow)
    to = np.full(grow, X, np.int32)
    idx.append_rows(ids[sl], coarse_id=to, codes=codes[sl]); model.append(ids[sl], to, codes[sl])
    assert model.list_len(X) > 256 * 64
    rng = np.random.default_rng(8)
    qrows = np.concatenate([rng.choice(n0, 16, replace=False), np.nonzero(cell[:n0] == X)[0][:4], [n0 + 5, n0 + 4000, n0 + 9000, n0 + 16000]])
    qs = np.ascontiguousarray(x[qrows])
    _remove(idx, model, model.list_ids[X][::3].copy(), "every third row")
    assert model.list_len(X) > 170 * 64
    _same_bytes(idx, gpu.IVFIndex, model, "ivf: thinned long list")
    tm._ivf_check(gpu, oracle, idx, model, qs, True, True, "ivf: a list of more than 256 blocks thinned by every third row")
    _remove(idx, model, model.list_ids[X][64:].copy(), "down to one block")
    tm._ivf_check(gpu, oracle, idx, model, qs, True, True, "ivf: the long list down to one block")
    idx.close()


def test_ivf_two_replicas_remove_append_remove(gpu, oracle):
    """freddy_gpu_pin_ivf_multi with the same device twice: remove_rows acts on every replica; a batch is split over both."""
    coarse, cb, ids, cell, codes, x = tm._ivf_source(300, 12, 256, 32)
    n0, n1 = 2000, 2400
    model = rm.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    idx = gpu.IVFIndex(*model.pin_args(), devices=[0, 0])
    assert idx.replicas == 2
    qs = np.ascontiguousarray(x[np.r_[10:30, n0:n0 + 20]])
    gone = []
    for step in ("rm", "append", "rm"):
        if step == "append":
            sl = slice(n0, n1)
            idx.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]); model.append(ids[sl], cell[sl], codes[sl])
        else:
            c = int(np.argmax([model.list_len(c) for c in range(32)]))
            few = ids[12:15] if not gone else ids[22:25]
            want = np.concatenate([model.list_ids[c][:1], model.list_ids[c][63:64], model.list_ids[c][64:128], [model.max_id], few])
            gone.append(np.unique(want)); _remove(idx, model, want, "replicas " + step)
        ot = model.oracle_table(oracle)
        fresh = gpu.IVFIndex(*model.pin_args())
        for fused in (1, 0):
            idx.set_option("fused", fused); fresh.set_option("fused", fused)
            got = idx.search(qs, 5, 3)
            util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(ot, qs, 5, 3), f"two replicas {step} fused={fused}")
            tm._bits_equal(got, fresh.search(qs, 5, 3), f"two replicas {step} fused={fused}")
            assert not np.isin(got[0], np.concatenate(gone)).any()
        fresh.close()
    assert idx.bound_violations() == 0
    idx.close()


# =======================================================================================
# 2. flat PQ
# =======================================================================================
PQ_CASES = [((300, 12, 256), 4200), ((35, 7, 16), 700)]


@pytest.mark.parametrize("shape,n0", PQ_CASES, ids=["300x12x256", "35x7x16"])
def test_pq_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, shape, n0):
    """Rows 5..39 and six rows around the end of the pinned table carry the codes of one other row: equal distances, so the
    lists are decided by the row order that the compaction has to keep.  After every step: one query, a batch (the shadow is
    rebuilt), a subset (the sub-view), grouping."""
    d, m, K = shape
    std = shape == (300, 12, 256)
    cb, ids, codes, x = tm._pq_source(d, m, K)
    codes = codes.copy()
    codes[5:40] = codes[4]; codes[n0 - 3:n0 + 3] = codes[100]
    rng = np.random.default_rng(m + K)
    total = n0 + 130
    qrows = np.concatenate([[4, 100], rng.choice(n0, 14, replace=False), rng.choice(np.arange(n0, total), 3, replace=False), [total - 1]])
    qs = np.ascontiguousarray(x[qrows])
    gv = np.ascontiguousarray(x[rng.choice(total, 5, replace=False)]); gv[3] = gv[0]
    model = rm.PQModel(cb, ids[:n0], codes[:n0])
    idx = gpu.PQIndex(*model.pin_args())
    sub = np.concatenate([ids[rng.choice(n0, 300, replace=False)], ids[n0:total:3], ids[:45], [1, 3, -5, 10 ** 8 + 1]]).astype(np.int32)

    def check(what, full=True):
        _same_bytes(idx, gpu.PQIndex, model, what)
        if full:
            tm._pq_check(gpu, oracle, idx, model, qs, sub, gv, std, what)
        else:
            fresh = gpu.PQIndex(*model.pin_args())
            for q in (qs[:1], qs):
                tm._bits_equal(idx.search(q, 5), fresh.search(q, 5), what)
            tm._bits_equal(idx.search(qs, 5, sentinel=1000.0, subset_ids=sub), fresh.search(qs, 5, sentinel=1000.0, subset_ids=sub), what)
            fresh.close()

    idx.search(qs, 7)                                   # the shadow exists before the first removal
    _remove(idx, model, np.concatenate([ids[:1], ids[63:64], ids[128:192], ids[7:9]]), "block edges")
    check("pq: lane 0, lane 63, a middle block")
    cb2 = tm._nudged(model.codebook, 55)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    edge = (model.N - 1) // 64 * 64                     # N -> 64 j + 1 -> 64 j -> 64 j - 1
    _remove(idx, model, model.ids[edge + 1:].copy(), "to 64 j + 1"); assert model.N == edge + 1
    check("pq: 64 j + 1 rows", full=False)
    _remove(idx, model, model.ids[100:101].copy(), "to 64 j"); assert model.N % 64 == 0
    check("pq: 64 j rows", full=False)
    _remove(idx, model, model.ids[-1:].copy(), "to 64 j - 1")
    check("pq: 64 j - 1 rows")
    idx.append_rows(ids[n0:total], codes=codes[n0:total]); model.append(ids[n0:total], codes[n0:total])
    last = int(model.ids[-1])
    _remove(idx, model, np.concatenate([ids[n0:n0 + 50], [last], model.ids[200:230]]), "appended rows")
    idx.append_rows([last - 1], codes=codes[7:8]); model.append([last - 1], codes[7:8])   # between the new and the old maximum
    check("pq: appended rows removed, an id above the one that was left")
    before, nbytes = [idx.search(qs[:1], 5), idx.search(qs, 5), idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)], idx.nbytes
    bad = np.array([-1, int(model.ids[3])], np.int32)
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*id -1 at position 0"):
        idx.remove_rows(bad)
    with pytest.raises(rm.Refused):
        model.remove(bad)
    gpu._check(idx.lib.freddy_gpu_remove_rows(idx.h, 0, None, None))
    assert idx.remove_rows([1, 3] + UNKNOWN) == 0 and idx.nbytes == nbytes and idx.N == model.N
    for a, b in zip(before, [idx.search(qs[:1], 5), idx.search(qs, 5), idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)]):
        tm._bits_equal(a, b, "pq: after the refused call")
    _remove(idx, model, model.ids.copy(), "every row")
    assert idx.N == 0
    check("pq: empty", full=False)
    refill = slice(40, 40 + (4200 if std else 400))     # (64 blocks and more: the shape pq_one_kernel serves, which _pq_check expects)
    idx.append_rows(ids[refill], codes=codes[refill]); model.append(ids[refill], codes[refill])
    check("pq: appended to the emptied handle")
    idx.close()


# =======================================================================================
# 3. kNN-join
# =======================================================================================
@pytest.mark.parametrize("std", [True, False], ids=["300x30x32xkc8", "64x8x16xkc4"])
@pytest.mark.parametrize("with_vectors", [True, False], ids=["vectors", "codes-only"])
def test_ivpq_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, std, with_vectors):
    """Both ends trimmed (ids stay consecutive: the O(1) id -> row rule with a new first id), a middle row (ids_affine turns
    false), an append, a swap, a scattered tenth of the rows, every row.  The join is called with the SAME target array
    immediately before and after the first removals: the cached "id IN (targets)" resolution must be dropped."""
    t, x = tm._ivpq_source(std)
    n0 = 3000
    vec = t["vectors"] if with_vectors else None
    take = lambda a, sl: None if a is None else a[sl]
    ids = t["ids"]
    model = rm.IVPQModel(t["codebook"], t["coarse"], ids[:n0], t["coarse_id"][:n0], t["codes"][:n0], take(vec, slice(0, n0)), t["stats"])
    idx = gpu.IVPQIndex(*model.pin_args())
    assert model.ids_affine
    rng = np.random.default_rng(32)
    qrows = np.concatenate([rng.choice(n0, 10, replace=False), [0, 1, n0 - 1, 1500, n0 + 2, n0 + 60]])
    qs = np.ascontiguousarray(x[qrows])
    targets = np.concatenate([ids[rng.choice(n0, 500, replace=False)], ids[:40], ids[n0 - 40:n0 + 65], ids[1490:1510], ids[:20], [10 ** 8, -4]]).astype(np.int32)
    methods = (0, 1, 2) if with_vectors else (0,)

    def check(what):
        _same_bytes(idx, gpu.IVPQIndex, model, what)
        ot = model.oracle_table(oracle)
        fresh = gpu.IVPQIndex(*model.pin_args())
        for method in methods:
            for tl in (True, False):
                for k, alpha, pvf, conf in tm.JOIN_CALLS:
                    w = f"{what} method={method} tl={tl} k={k} alpha={alpha}"
                    gi, gd, git = idx.knn_join(qs, k, targets, alpha, pvf, method, use_target_lists=tl, confidence=conf)
                    exp, eit = oracle.ivpq_search_in(ot, qs, k, targets, alpha, pvf, method, use_target_lists=tl, confidence=conf)
                    assert git == eit, (w, git, eit)
                    util.assert_same_lists(gi, gd, exp, w)
                    fi, fd, fit = fresh.knn_join(qs, k, targets, alpha, pvf, method, use_target_lists=tl, confidence=conf)
                    tm._bits_equal((gi, gd), (fi, fd), w)
                    assert fit == git, w
        fresh.close()

    def same_targets(what, ids_gone):
        got = idx.knn_join(qs, 5, targets, 3, 20, methods[-1])
        exp, eit = oracle.ivpq_search_in(model.oracle_table(oracle), qs, 5, targets, 3, 20, methods[-1])
        assert got[2] == eit, what
        util.assert_same_lists(got[0], got[1], exp, what)
        assert not np.isin(got[0], ids_gone).any(), what
        return got

    before = same_targets("before", [])
    ends = np.concatenate([ids[:7], ids[n0 - 5:n0]])
    assert np.isin(before[0], ends).any(), "no row that is about to leave among the results: the case does not bite"
    _remove(idx, model, ends, "both ends"); assert model.ids_affine
    same_targets("the same targets after the ends went", ends)
    check("ivpq: both ends trimmed")
    mid = ids[1500:1501]
    _remove(idx, model, mid, "a middle row"); assert not model.ids_affine
    same_targets("the same targets after a middle row went", np.concatenate([ends, mid]))
    check("ivpq: a middle row")
    sl = slice(n0, n0 + 65)
    idx.append_rows(ids[sl], coarse_id=t["coarse_id"][sl], codes=t["codes"][sl], vectors=take(vec, sl))
    model.append(ids[sl], t["coarse_id"][sl], t["codes"][sl], take(vec, sl))
    cb2 = tm._nudged(model.codebook, 401)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    idx.set_option("join_host_traversal", 1)
    _remove(idx, model, np.concatenate([model.ids[rng.choice(model.N, 300, replace=False)], ids[n0 + 60:n0 + 65]]), "a tenth")
    same_targets("host traversal after a tenth went", [])
    idx.set_option("join_host_traversal", 0)
    check("ivpq: a tenth of the rows, appended ones among them")
    nbytes = idx.nbytes
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*id -7 at position 1"):
        idx.remove_rows([int(model.ids[0]), -7])
    assert idx.remove_rows(UNKNOWN) == 0 and idx.nbytes == nbytes and idx.N == model.N
    same_targets("after the refused call", [])
    _remove(idx, model, model.ids.copy(), "every row")
    _same_bytes(idx, gpu.IVPQIndex, model, "ivpq: empty")
    sl = slice(100, 700)
    idx.append_rows(ids[sl], coarse_id=t["coarse_id"][sl], codes=t["codes"][sl], vectors=take(vec, sl))
    model.append(ids[sl], t["coarse_id"][sl], t["codes"][sl], take(vec, sl))
    assert model.ids_affine
    check("ivpq: appended to the emptied handle")
    idx.close()


# =======================================================================================
# 4. raw vectors
# =======================================================================================
def _vec_more(gpu, idx, model, qs, sub, what):
    """exact join and assign against a fresh pin (exact search and the analogies: tm._vec_check) -> the fresh pin's footprint"""
    fresh = gpu.VectorIndex(*model.pin_args())
    for mode in (1, -1):
        idx.set_option("exact_filter", mode); fresh.set_option("exact_filter", mode)
        tm._bits_equal(idx.join(qs, 5, sub), fresh.join(qs, 5, sub), what + " join")
        tm._bits_equal(idx.join(qs, 5, sub), idx.search(qs, 5, subset_ids=sub), what + " join vs subset search")
        tm._bits_equal(idx.assign(qs, sub), fresh.assign(qs, sub), what + " assign")
    lo = fresh.nbytes
    fresh.close()
    return lo


@pytest.mark.parametrize("d", [300, 64, 35])
def test_vec_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, d):
    """194 rows: a middle row (193), the first row (192 = three 64-row blocks = six 32-row strips), the last row (191), 31
    scattered rows (160 = five strips), one more (159), an append, every row, an append.  exact_filter = 1 keeps the fragment
    copy in use where the shape has it (d = 35 has none)."""
    n0, total = 194, 400
    x, ids = tm._vec_table(d, total)
    rng = np.random.default_rng(d)
    qs, triples, sub = tm._vec_queries(x, ids, n0, total, rng)
    model = rm.VecModel(ids[:n0], x[:n0])
    idx = gpu.VectorIndex(*model.pin_args())
    nbytes = idx.nbytes

    def check(what):
        nonlocal nbytes
        lo = _vec_more(gpu, idx, model, qs, sub, what)
        assert lo <= idx.nbytes <= nbytes, (what, "freddy_gpu_index_bytes", lo, idx.nbytes, nbytes)
        nbytes = idx.nbytes
        names, _ = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, what, modes=(1, -1))
        assert ("exact_filter" in names) == (d != 35), (what, sorted(names))

    steps = [("a middle row", lambda: model.ids[97:98]), ("the first row", lambda: model.ids[:1]), ("the last row", lambda: model.ids[-1:]),
             ("31 scattered rows", lambda: model.ids[rng.choice(model.N, 31, replace=False)]), ("one more", lambda: model.ids[64:65])]
    for (what, pick), n_after in zip(steps, (193, 192, 191, 160, 159)):
        _remove(idx, model, pick().copy(), what)
        assert model.N == n_after
        check(f"vec d={d}: {what}, N={n_after}")
    idx.append_rows(ids[n0:n0 + 100], vectors=x[n0:n0 + 100]); model.append(ids[n0:n0 + 100], x[n0:n0 + 100])
    nbytes = idx.nbytes
    _remove(idx, model, np.concatenate([ids[n0:n0 + 40], model.ids[:3]]), "appended rows")
    check(f"vec d={d}: appended rows removed")
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*id -2 at position 1"):
        idx.remove_rows([int(model.ids[0]), -2])
    assert idx.remove_rows([4] + UNKNOWN) == 0 and idx.nbytes == nbytes and idx.N == model.N
    _remove(idx, model, model.ids.copy(), "every row")
    fresh = gpu.VectorIndex(*model.pin_args())
    tm._bits_equal(idx.search(qs, 5), fresh.search(qs, 5), "vec: empty")
    assert fresh.nbytes <= idx.nbytes <= nbytes
    fresh.close()
    idx.append_rows(ids[200:330], vectors=x[200:330]); model.append(ids[200:330], x[200:330])
    nbytes = max(nbytes, idx.nbytes)
    check(f"vec d={d}: appended to the emptied handle")
    idx.close()


def test_vec_the_row_with_the_largest_element_leaves_and_the_scale_comes_back(gpu, oracle):
    """One row 300 times as long as any other decides the power-of-two scale of the fragment copy.  With it gone the statistics are
    taken again over the rows that are left: a fresh pin's scale and norm bound (the float bits of the filter path agree with
    a fresh pin, every row refined: no bracket violated)."""
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n)
    x[4000] *= np.float32(300.0)
    rng = np.random.default_rng(9)
    qs, triples, sub = tm._vec_queries(x, ids, 8000, n, rng)
    model = rm.VecModel(ids, x)
    idx = gpu.VectorIndex(*model.pin_args())
    names, passes = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, "with the long row", modes=(-1,))
    assert "exact_filter" in names and passes > 0
    nbytes = idx.nbytes
    _remove(idx, model, ids[4000:4001], "the long row")
    names, passes = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, "without the long row", modes=(-1,))
    assert "exact_filter" in names and passes > 0
    lo = _vec_more(gpu, idx, model, qs, sub, "without the long row")
    assert lo <= idx.nbytes <= nbytes
    idx.set_option("check_brackets", 4 | 8)
    before = idx.bound_checked()
    tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, "without the long row, every row refined", modes=(-1,))
    assert idx.bound_checked() - before >= len(qs) * model.N and idx.bound_violations() == 0
    idx.close()


def test_vec_the_only_non_finite_row_leaves_and_the_filter_is_back(gpu, oracle):
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n)
    x[123, 5] = np.float32(np.inf)
    good = np.r_[0:123, 124:n]
    rng = np.random.default_rng(10)
    qs = np.ascontiguousarray(x[rng.choice(good, 10, replace=False)])
    model = rm.VecModel(ids, x)
    idx = gpu.VectorIndex(*model.pin_args())
    idx.set_option("exact_filter", 1)
    _, names = tm._profiled(idx, lambda: idx.search(qs, 5))
    assert "exact_filter" not in names and "exact_scan" in names, sorted(names)
    _remove(idx, model, ids[123:124], "the non-finite row")
    (gi, gs), names = tm._profiled(idx, lambda: idx.search(qs, 5))
    assert "exact_filter" in names, sorted(names)
    tm._exact_same(gi, gs, [oracle.exact_knn(model.vectors, model.ids, q, 5) for q in qs], 5, "the non-finite row gone")
    fresh = gpu.VectorIndex(*model.pin_args())
    fresh.set_option("exact_filter", 1)
    tm._bits_equal((gi, gs), fresh.search(qs, 5), "the non-finite row gone")
    assert idx.nbytes == fresh.nbytes and idx.bound_violations() == 0   # (the fragment copy was allocated by the removal: a fresh pin's size)
    fresh.close(); idx.close()


def test_vec_pinned_without_the_filter_stays_without_it(gpu, oracle, monkeypatch):
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n)
    monkeypatch.setenv("FREDDY_GPU_EXACT_FILTER", "0")
    model = rm.VecModel(ids, x)
    idx = gpu.VectorIndex(*model.pin_args())
    monkeypatch.delenv("FREDDY_GPU_EXACT_FILTER")
    nbytes = idx.nbytes
    qs = np.ascontiguousarray(x[[3, 500, 8000]])
    idx.set_option("exact_filter", 1)
    _remove(idx, model, ids[50:60], "ten rows")
    for mode in (1, -1):
        idx.set_option("exact_filter", mode)
        (gi, gs), names = tm._profiled(idx, lambda: idx.search(qs, 5))
        assert "exact_filter" not in names and "exact_scan" in names, (mode, sorted(names))
        tm._exact_same(gi, gs, [oracle.exact_knn(model.vectors, model.ids, q, 5) for q in qs], 5, f"pinned without the filter, option {mode}")
    assert idx.nbytes < nbytes, "a fragment copy appeared"
    idx.close()


# =======================================================================================
# 5. the host mirror
# =======================================================================================
def _session(x, ids_all, pq, ivf, cell_of, iv, keep):
    from freddy_amd import udf
    s = udf.Session()
    s.load_vecs_norm(ids_all[keep], x[keep])
    k = np.isin(pq["ids"], ids_all[keep]); s.load_pq(pq["codebook"], pq["ids"][k], pq["codes"][k])
    k = np.isin(ivf["ids"], ids_all[keep]); s.load_ivfadc(ivf["coarse"], ivf["codebook"], ivf["ids"][k], cell_of[k], ivf["codes"][k])
    k = np.isin(iv["ids"], ids_all[keep]); s.load_ivpq(iv["codebook"], iv["coarse"], iv["ids"][k], iv["coarse_id"][k], iv["codes"][k], iv["stats"])
    return s


def test_delete_rows_then_insert_batch_equal_a_session_loaded_from_the_remaining_rows(gpu):
    """delete_rows on a session with every table loaded and the vector handle pinned; then every UDF family answers as a session
    loaded from the rows that are left -- and again after an insert_batch on both (the new ids start above the largest id
    that is LEFT in each table)."""
    N = 20000
    x = util.corpus(N).numpy()
    ids_all = np.arange(1, N + 1, dtype=np.int32)
    pq, ivf, iv = util.pq_tables(N=N, K=256), util.ivf_tables(N=N, C=32, K=256), util.ivpq_tables(N=N)
    cell_of = np.repeat(np.arange(32), np.diff(ivf["list_off"])).astype(np.int32)
    rng = np.random.default_rng(12)
    gone = np.concatenate([rng.choice(ids_all[:N - 50], 700, replace=False), ids_all[N - 20:], [1, 64, 65]]).astype(np.int32)
    keep = ~np.isin(ids_all, gone)
    a = _session(x, ids_all, pq, ivf, cell_of, iv, np.ones(N, bool))
    q = x[123]
    a.k_nearest_neighbour(q, 3)                         # google_vecs_norm is pinned before the rows leave
    ask = np.concatenate([gone, gone[:5], [N + 5]]).astype(np.int32)
    assert a.delete_rows(ask) == np.unique(gone).size
    assert a.delete_rows(ask) == 0
    b = _session(x, ids_all, pq, ivf, cell_of, iv, keep)
    qids = np.concatenate([ids_all[keep][[5, 900, 15000]], gone[:2]]).astype(np.int32)
    qs = x[[77, 4000, 123]]
    targets = np.concatenate([ids_all[::13], gone[:50]]).astype(np.int32)

    def same(what):
        for s_q in (q, x[int(gone[0]) - 1]):
            for name, call in (("pq_search", lambda s: s.pq_search(s_q, 6)), ("ivfadc_search", lambda s: s.ivfadc_search(s_q, 6)),
                               ("pq_search_in", lambda s: s.pq_search_in(s_q, 4, targets)), ("k_nearest_neighbour", lambda s: s.k_nearest_neighbour(s_q, 5)),
                               ("knn_in_exact", lambda s: s.knn_in_exact(s_q, 5, targets))):
                ra, rb = call(a), call(b)
                assert ra.tobytes() == rb.tobytes(), (what, name)
                assert not np.isin(ra["id"], gone).any(), (what, name)
        ra, rb = a.ivfadc_batch_search(qids, 5), b.ivfadc_batch_search(qids, 5)
        assert ra.tobytes() == rb.tobytes() and not np.isin(ra["query_id"], gone).any(), (what, "ivfadc_batch_search")
        three = np.arange(1, 4, dtype=np.int32)
        for method in (0, 2):
            ra = a.ivpq_search_in(qs, three, 4, targets, 3, 5, method, True, 0.8, 10000000)
            rb = b.ivpq_search_in(qs, three, 4, targets, 3, 5, method, True, 0.8, 10000000)
            assert ra.tobytes() == rb.tobytes(), (what, "ivpq_search_in", method)
        ra, rb = a.pq_search_in_batch(qs, three, 5, targets, True), b.pq_search_in_batch(qs, three, 5, targets, True)
        assert ra.tobytes() == rb.tobytes(), (what, "pq_search_in_batch")

    same("after delete_rows")
    v = x[rng.choice(N, 9, replace=False)] * np.float32(0.999)
    na, nb = a.insert_batch(v), b.insert_batch(v)
    assert na.tolist() == nb.tolist() == list(range(N - 19, N - 10)), (na, nb)
    same("after insert_batch")
    # the inserted rows are there: google_vecs_norm knows the new ids as queries, the flat table finds them as a subset
    assert sorted(set(a.ivfadc_batch_search(na[:2], 5)["query_id"].tolist())) == na[:2].tolist()
    assert set(a.pq_search_in(v[0], 3, na)["id"][:3].tolist()) <= set(na.tolist()) and a.pq_search_in(v[0], 3, na)["id"][0] >= N - 19
    a.close(); b.close()
