"""-m gpu: freddy_gpu_update_rows, the fourth way a pinned handle changes -- a row keeps its id and gets a new payload -- in
sequences that mix it with append_rows, remove_rows and update_codebook on every handle kind.  tests/update_model.py applies
every step to host arrays; after every step the checks of tests/test_gpu_mutation.py for that kind compare the handle with the
CPU oracle on the model's tables (ids, ranks, distance bits) and with a FRESH pin of them (ids and float bits, the kernel that
served each call, bound_violations() == 0), and freddy_gpu_index_bytes with the fresh pin's.  Nothing here has a tolerance.

What is updated is chosen by the layouts' edges: scattered lanes of a list of three blocks and more, lane 0 and lane 63 of a
block of appended rows, a row that changes its list, a list going 65 -> 64 -> 63 rows by moves out and back to 65 by moves in, a
whole cell moved away (a second probing round) and refilled, the row with the largest id, one row twice, appended rows, every
row in one call; the first row of a 32-row strip, lane 63 of a 64-row block and the last row of a vector table, the row with the
largest element, a row that turns non-finite and back.  Every sequence asserts on the CPU, from the oracle's lists alone, that
an update changed some query's answer: an updated row was a query's neighbour and its new payload puts it elsewhere."""
import numpy as np
import pytest

import pv_model as pm
import test_gpu_mutation as tm
import test_gpu_nonfinite as tn
import test_gpu_removal as tr
import update_model as um
import util

pytestmark = pytest.mark.gpu

E_ARG = tm.E_ARG
UNKNOWN = tr.UNKNOWN


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _shuffled(n, *arrays):
    order = np.random.default_rng(n + 1).permutation(n)
    return [None if a is None else np.ascontiguousarray(np.asarray(a)[order]) for a in arrays]


def _with_unknown(ids, *payload):
    """two ids no table has, with payloads of their own (copies of the first rows'), then everything shuffled"""
    ids = np.concatenate([np.asarray(ids, np.int64).reshape(-1), UNKNOWN])
    payload = [None if a is None else np.concatenate([np.asarray(a), np.asarray(a)[:1], np.asarray(a)[:1]]) for a in payload]
    return _shuffled(ids.size, ids, *payload)


def _ids_differ(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b))


# =======================================================================================
# 1. IVFADC
# =======================================================================================
def _ivf_update(idx, model, ids, cell, codes, what):
    """the same rows (shuffled, unknown ids among them) to the handle and to the model: equal counts, N and max_id as before"""
    ids = np.asarray(ids).reshape(-1)
    n, top = model.N, model.max_id
    a_ids, a_cell, a_codes = _with_unknown(ids, cell, codes)
    got, exp = idx.update_rows(a_ids, coarse_id=a_cell, codes=a_codes), model.update(a_ids, a_cell, a_codes)
    assert got == exp == ids.size, (what, got, exp, ids.size)
    assert idx.N == model.N == n and model.max_id == top, what


@pytest.mark.parametrize("shape", tr.IVF_CASES, ids=["300x12x256x32", "300x12x1024x32", "100x5x64x16"])
def test_ivf_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, shape):
    d, m, K, C = shape
    special = m == 12 and d == 300
    coarse, cb, ids, cell, codes, x, n_big = tr._ivf_rows(shape)
    n0 = n_big + 2600
    n1 = n0 + 300
    spare = np.arange(n1, ids.size)                      # rows that are never pinned: their (cell, codes) are the new payloads
    model = um.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    idx = gpu.IVFIndex(*model.pin_args())
    by_len = [int(c) for c in np.argsort([-model.list_len(c) for c in range(C)], kind="stable")]
    A, B, D, E = by_len[0], by_len[1], by_len[2], by_len[3]
    assert model.list_len(A) >= 193 and model.list_len(B) >= 193 and model.list_len(D) >= 66
    rng = np.random.default_rng(K + C + 1)
    in_E = np.nonzero(cell[:n0] == E)[0]
    qrows = np.concatenate([rng.choice(n0, 30, replace=False), in_E[:3], [n0 + 3, n0 + 250]])
    qs = np.ascontiguousarray(x[qrows])
    assert (oracle.assign_coarse(coarse, qs) == E).any(), "no query probes the cell that will be emptied"
    la, lb, ld = model.list_ids[A].copy(), model.list_ids[B].copy(), model.list_ids[D].copy()
    lists = lambda: oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3)["id"].copy()
    take = iter(spare)
    src = lambda n: np.array([next(take) for _ in range(n)])   # n fresh payload rows

    def check(what, full=True):
        tr._same_bytes(idx, gpu.IVFIndex, model, what)
        if full:
            tm._ivf_check(gpu, oracle, idx, model, qs, special, K <= 256, what)
        else:
            fresh = gpu.IVFIndex(*model.pin_args())
            for q in (qs, qs[-1:]):
                got = idx.search(q, 5, 3)
                util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(model.oracle_table(oracle), q, 5, 3), what)
                tm._bits_equal(got, fresh.search(q, 5, 3), what)
            fresh.close()

    def move(rows_ids, to, what, full=False):
        s = src(len(rows_ids))
        _ivf_update(idx, model, rows_ids, np.full(len(rows_ids), to, np.int32), codes[s], what)
        check("ivf: " + what, full)

    # codes only, in scattered lanes of lists of three blocks and more (a fresh pin arranges a list's rows for the LDS banks)
    pick = np.concatenate([la[3::7], lb[:1], lb[127:129]])
    _ivf_update(idx, model, pick, model.cell_of(pick), codes[src(pick.size)], "scattered lanes")
    check("ivf: new codes in scattered lanes of lists of three blocks")
    # the queries' nearest rows get the payload of rows elsewhere: they change their lists, and the answers change
    before = lists()
    near = np.unique(before[:6, 0])
    s = src(near.size)
    s_cell = np.where(cell[s] == model.cell_of(near), (cell[s] + 1) % C, cell[s]).astype(np.int32)
    _ivf_update(idx, model, near, s_cell, codes[s], "neighbours move away")
    assert _ids_differ(before, lists()), "the update changed no list: the case does not bite"
    check("ivf: the nearest rows of six queries moved to other lists")
    la, lb, ld = model.list_ids[A].copy(), model.list_ids[B].copy(), model.list_ids[D].copy()   # (the lists as they are now, in id order)
    assert ld.size >= 66
    # a list going 65 -> 64 -> 63 by moves out and 63 -> 64 -> 65 by moves in
    move(ld[65:], B, "a list down to 65 rows"); assert model.list_len(D) == 65
    move(ld[10:11], A, "65 -> 64 by a move out"); assert model.list_len(D) == 64
    move(ld[64:65], A, "64 -> 63 by a move out"); assert model.list_len(D) == 63
    move(la[1:2], D, "63 -> 64 by a move in"); assert model.list_len(D) == 64
    move(la[2:3], D, "64 -> 65 by a move in", full=True); assert model.list_len(D) == 65
    # every row of a cell moved away: the queries nearest to it go into a second probing round; then rows move into the empty cell
    e_rows = model.list_ids[E].copy()
    move(e_rows, A, "a whole cell moved away", full=True)
    near_cell = oracle.assign_coarse(coarse, qs)
    assert model.list_len(E) == 0 and sum(1 for c in near_cell if model.list_len(int(c)) < 30) > 0
    move(e_rows[:5], E, "rows moved into the empty cell"); assert model.list_len(E) == 5
    # after update_codebook
    cb2 = tm._nudged(model.codebook, 78)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    pick = lb[5::9]
    _ivf_update(idx, model, pick, model.cell_of(pick), codes[src(pick.size)], "after the swap")
    check("ivf: new codes after update_codebook")
    # appended rows: the first 70 go to list D behind its 65 rows, so row 62 takes lane 63 of block 1 and row 63 lane 0 of block 2
    sl = slice(n0, n1)
    to = cell[sl].copy(); to[:70] = D
    idx.append_rows(ids[sl], coarse_id=to, codes=codes[sl]); model.append(ids[sl], to, codes[sl])
    assert model.list_len(D) >= 135           # (the 70 come first: their places behind the 65 rows do not depend on the others)
    edge = ids[n0 + 62:n0 + 64]
    _ivf_update(idx, model, edge, [D, D], codes[src(2)], "lane 63 and lane 0 of blocks of appended rows")
    check("ivf: lane 63 and lane 0 of blocks of appended rows", full=False)
    late = ids[n0 + 100:n0 + 140]
    s = src(late.size)
    _ivf_update(idx, model, late, cell[s], codes[s], "appended rows")
    gone = np.concatenate([late[::2], near[:2], edge[:1]])
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    check("ivf: appended rows updated, then updated rows removed")
    # the row with the largest id: max_id ends as it began
    top = model.max_id
    assert top == int(ids[n1 - 1])
    s = src(1)
    _ivf_update(idx, model, [top], (model.cell_of([top]) + 1) % C, codes[s], "the largest id")
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*largest pinned id"):
        idx.append_rows([top], coarse_id=[0], codes=codes[s])
    with pytest.raises(um.Refused):
        model.append([top], [0], codes[s])
    idx.append_rows([top + 1], coarse_id=[E], codes=codes[s]); model.append([top + 1], [E], codes[s])
    check("ivf: the row with the largest id updated, then an append right above it", full=False)
    # the same row in two consecutive calls: the last wins
    s = src(2)
    for j in range(2):
        _ivf_update(idx, model, la[5:6], [(A, B)[j]], codes[s[j:j + 1]], f"the same row, call {j}")
    assert int(model.cell_of(la[5:6])[0]) == B
    check("ivf: the same row updated twice", full=False)
    # refused: the answers, the footprint and the row count stay
    answers = lambda: [idx.search(qs, 5, 3), idx.search(qs[:1], 5, 3)]
    was, nbytes, n_rows = answers(), idx.nbytes, idx.N
    two, c2, k2 = la[40:42].astype(np.int32), np.array([A, B], np.int32), codes[src(2)]
    bad_code = k2.copy(); bad_code[1, m - 1] = K
    for args, words in (((np.array([la[40], la[41], la[40]]), [A, B, A], codes[:3]), rf"id {int(la[40])} is listed twice, at positions 0 and 2"),
                        ((np.array([la[40], -3]), c2, k2), r"id -3 at position 1"),
                        ((two, [A, C], k2), rf"coarse_id {C} of update row 1 "),
                        ((two, [-1, B], k2), r"coarse_id -1 of update row 0 "),
                        ((two, c2, bad_code), rf"code {K} of update row 1 position {m - 1} "),
                        ((two, None, k2), r"required"), ((two, c2, None), r"required")):
        with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*" + words):
            idx.update_rows(args[0], coarse_id=args[1], codes=args[2])
        with pytest.raises(um.Refused):
            model.update(*args)
    gpu._check(idx.lib.freddy_gpu_update_rows(idx.h, 0, None, None, None, None, None))
    assert idx.update_rows(UNKNOWN, coarse_id=[A, B], codes=k2) == model.update(UNKNOWN, [A, B], k2) == 0
    assert idx.nbytes == nbytes and idx.N == model.N == n_rows
    for a, b in zip(was, answers()):
        tm._bits_equal(a, b, "ivf: after the refused calls")
    # every row in one call, the cells permuted
    all_ids = np.concatenate(model.list_ids)
    perm = np.roll(np.arange(C), 1).astype(np.int32)
    before = lists()
    s = rng.choice(spare, all_ids.size)
    _ivf_update(idx, model, all_ids, perm[model.cell_of(all_ids)], codes[s], "every row")
    assert _ids_differ(before, lists())
    check("ivf: every row in one call, the cells permuted")
    idx.close()


def test_ivf_two_replicas_follow_an_update(gpu, oracle):
    """freddy_gpu_pin_ivf_multi with the same device twice: update_rows acts on every replica; a batch is split over both."""
    coarse, cb, ids, cell, codes, x = tm._ivf_source(300, 12, 256, 32)
    n0, n1 = 2000, 2400
    model = um.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    idx = gpu.IVFIndex(*model.pin_args(), devices=[0, 0])
    assert idx.replicas == 2
    qrows = np.r_[10:30, 1500:1520]
    qs = np.ascontiguousarray(x[qrows])
    lists = lambda: oracle.ivfadc_search_many(model.oracle_table(oracle), qs, 5, 3)["id"].copy()
    changed = False
    for step in ("update", "append", "update"):
        before = lists()
        if step == "append":
            sl = slice(n0, n1)
            idx.append_rows(ids[sl], coarse_id=cell[sl], codes=codes[sl]); model.append(ids[sl], cell[sl], codes[sl])
        else:   # the queries' own rows (both halves of the batch) get the payload of rows elsewhere; a few more keep their cell
            first = step == "update" and not changed
            mine = ids[qrows[::2]] if first else ids[qrows[1::2]]
            s = np.arange(3000, 3000 + mine.size) + (0 if first else 100)
            stay = model.list_ids[3][~np.isin(model.list_ids[3], ids[qrows])][:5]
            a_ids = np.concatenate([mine, stay])
            _ivf_update(idx, model, a_ids, np.concatenate([cell[s], model.cell_of(stay)]), codes[np.r_[s, 3500:3505]], "replicas " + step)
            changed |= _ids_differ(before, lists())
        ot = model.oracle_table(oracle)
        fresh = gpu.IVFIndex(*model.pin_args())
        for fused in (1, 0):
            idx.set_option("fused", fused); fresh.set_option("fused", fused)
            got = idx.search(qs, 5, 3)
            util.assert_same_lists(got[0], got[1], oracle.ivfadc_search_many(ot, qs, 5, 3), f"two replicas {step} fused={fused}")
            tm._bits_equal(got, fresh.search(qs, 5, 3), f"two replicas {step} fused={fused}")
        fresh.close()
    assert changed and idx.bound_violations() == 0
    idx.close()


# =======================================================================================
# 2. flat PQ
# =======================================================================================
def _pq_check_like_fresh(gpu, oracle, idx, model, qs, sub, gv, what):
    """tm._pq_check for a shape whose kernels that check does not name: the same calls, the oracle's lists, a fresh pin's bits and
    the fresh pin's kernel names"""
    ot = model.oracle_table(oracle)
    fresh = gpu.PQIndex(*model.pin_args())
    for one, fused in ((1, -1), (0, -1), (1, 1), (1, 0)):
        for h in (idx, fresh):
            h.set_option("one_launch", one); h.set_option("pq_fused", fused)
        for q, k in ((qs[:1], 5), (qs, 7)):
            got, names = tm._profiled(idx, lambda: idx.search(q, k, sentinel=100.0))
            exp_f, names_f = tm._profiled(fresh, lambda: fresh.search(q, k, sentinel=100.0))
            w = f"{what} one_launch={one} pq_fused={fused} Q={len(q)}"
            util.assert_same_lists(got[0], got[1], np.stack([oracle.pq_search(ot, v, k) for v in q]), w)
            tm._bits_equal(got, exp_f, w)
            assert names == names_f, (w, sorted(names), sorted(names_f))
    got = idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)
    util.assert_same_lists(got[0], got[1], oracle.pq_search_in_batch(ot, qs, 5, sub), f"{what} subset")
    tm._bits_equal(got, fresh.search(qs, 5, sentinel=1000.0, subset_ids=sub), f"{what} subset")
    for s in (None, sub):
        gi, gg = idx.grouping(gv, s)
        ei, eg = oracle.grouping_pq(ot, gv, model.ids if s is None else s)
        assert np.array_equal(gi, ei) and np.array_equal(gg, eg), (what, "grouping")
    fresh.close()


@pytest.mark.parametrize("shape,n0", [((300, 12, 256), 4200), ((300, 12, 1024), 4200), ((35, 7, 16), 700)], ids=["300x12x256", "300x12x1024", "35x7x16"])
def test_pq_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, shape, n0):
    """A batch of 20 queries before and after every update (a stale shadow would show), a subset (the sub-view), one query,
    grouping and the assignment step of cluster_pq."""
    d, m, K = shape
    std = shape == (300, 12, 256)
    cb, ids, codes, x = tm._pq_source(d, m, K)
    rng = np.random.default_rng(m + K + 1)
    total = n0 + 130
    spare = np.arange(total, total + 1500)
    qrows = np.concatenate([[4, 63, 64, n0 - 1], rng.choice(n0, 12, replace=False), rng.choice(np.arange(n0, total), 3, replace=False), [total - 1]])
    qs = np.ascontiguousarray(x[qrows])
    gv = np.ascontiguousarray(x[rng.choice(total, 5, replace=False)]); gv[3] = gv[0]
    model = um.PQModel(cb, ids[:n0], codes[:n0])
    idx = gpu.PQIndex(*model.pin_args())
    sub = np.concatenate([ids[rng.choice(n0, 300, replace=False)], ids[qrows[:4]], ids[n0:total:3], ids[:45], [1, 3, -5, 10 ** 8 + 1]]).astype(np.int32)
    lists = lambda: np.stack([oracle.pq_search(model.oracle_table(oracle), q, 7)["id"] for q in qs])
    take = iter(spare)
    src = lambda n: np.array([next(take) for _ in range(n)])

    def update(rows_ids, what):
        rows_ids = np.asarray(rows_ids).reshape(-1)
        a_ids, a_codes = _with_unknown(rows_ids, codes[src(rows_ids.size)])
        got, exp = idx.update_rows(a_ids, codes=a_codes), model.update(a_ids, a_codes)
        assert got == exp == rows_ids.size and idx.N == model.N, (what, got, exp)

    def check(what):
        tr._same_bytes(idx, gpu.PQIndex, model, what)
        if K == 1024:
            _pq_check_like_fresh(gpu, oracle, idx, model, qs, sub, gv, what)
        else:
            tm._pq_check(gpu, oracle, idx, model, qs, sub, gv, std, what)
        fresh = gpu.PQIndex(*model.pin_args())
        tm._bits_equal(idx.assign(qs, sub), fresh.assign(qs, sub), what + " pq_assign")
        fresh.close()

    idx.search(qs, 7); idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)     # the shadow and the sub-view exist before the first update
    before = lists()
    update(np.concatenate([ids[qrows[:4]], ids[128:131], ids[n0 - 2:n0 - 1]]), "block edges")   # lane 0, lane 63, the last row: queries' own rows
    assert _ids_differ(before, lists()), "the update changed no list: the case does not bite"
    check("pq: the queries' own rows at lane 0, lane 63 and the end of the table")
    cb2 = tm._nudged(model.codebook, 56)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    update(ids[rng.choice(n0, 200, replace=False)], "after the swap")
    check("pq: 200 rows after update_codebook")
    idx.append_rows(ids[n0:total], codes=codes[n0:total]); model.append(ids[n0:total], codes[n0:total])
    top = int(model.ids[-1])
    update(np.concatenate([ids[n0:n0 + 50], [top]]), "appended rows and the largest id")
    gone = np.concatenate([ids[n0:n0 + 20], ids[128:130]])
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*largest pinned id"):
        idx.append_rows([top], codes=codes[:1])
    idx.append_rows([top + 1], codes=codes[7:8]); model.append([top + 1], codes[7:8])
    for j in range(2):                                   # the same row twice: the last wins
        update(ids[300:301], f"the same row, call {j}")
    check("pq: appended rows updated, updated rows removed, an append above the same largest id, one row twice")
    # refused: the answers, the footprint and the row count stay
    answers = lambda: [idx.search(qs[:1], 5), idx.search(qs, 5), idx.search(qs, 5, sentinel=1000.0, subset_ids=sub)]
    was, nbytes, n_rows = answers(), idx.nbytes, idx.N
    two, k2 = ids[500:502], codes[src(2)]
    high = k2.copy(); high[0, 2] = K
    for args, words in (((np.array([ids[500], ids[501], ids[501]]), codes[:3]), rf"id {int(ids[501])} is listed twice, at positions 1 and 2"),
                        ((np.array([-1, ids[500]]), k2), r"id -1 at position 0"),
                        ((two, high), rf"code {K} of update row 0 position 2 "),
                        ((two, None), r"codes are required")):
        with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*" + words):
            idx.update_rows(args[0], codes=args[1])
        with pytest.raises(um.Refused):
            model.update(*args)
    gpu._check(idx.lib.freddy_gpu_update_rows(idx.h, 0, None, None, None, None, None))
    with pytest.raises(gpu.FreddyGpuError, match=rf"codes has {2 * (m - 1)} elements, 2 ids need {2 * m}"):
        idx.update_rows(two, codes=k2[:, :m - 1])         # (the binding: the library would read past the array)
    assert idx.lib.freddy_gpu_update_rows(idx.h, 2 ** 31, two.ctypes.data, None, k2.ctypes.data, None, None) == -5   # FREDDY_E_LIMIT, before anything is read
    assert b"at most" in idx.lib.freddy_gpu_last_error()
    assert idx.update_rows([1, 3] + UNKNOWN, codes=codes[:4]) == model.update([1, 3] + UNKNOWN, codes[:4]) == 0
    assert idx.nbytes == nbytes and idx.N == model.N == n_rows
    for a, b in zip(was, answers()):
        tm._bits_equal(a, b, "pq: after the refused calls")
    before = lists()
    a_ids, a_codes = _shuffled(model.N, model.ids, codes[rng.choice(spare, model.N)])
    assert idx.update_rows(a_ids, codes=a_codes) == model.update(a_ids, a_codes) == model.N
    assert _ids_differ(before, lists())
    check("pq: every row in one call")
    idx.close()


# =======================================================================================
# 3. kNN-join
# =======================================================================================
@pytest.mark.parametrize("std", [True, False], ids=["300x30x32xkc8", "64x8x16xkc4"])
@pytest.mark.parametrize("with_vectors", [True, False], ids=["vectors", "codes-only"])
def test_ivpq_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, std, with_vectors):
    """The join is called with target lists on and the SAME target array immediately before and after an update that changes
    cells: the cached "id IN (targets)" resolution is bucketed by cell and must be dropped.  Methods 1 and 2 read the vectors."""
    t, x = tm._ivpq_source(std)
    n0 = 3000
    vec = t["vectors"] if with_vectors else None
    take_v = lambda rows: None if vec is None else vec[rows]
    ids = t["ids"]
    model = um.IVPQModel(t["codebook"], t["coarse"], ids[:n0], t["coarse_id"][:n0], t["codes"][:n0], take_v(slice(0, n0)), t["stats"])
    idx = gpu.IVPQIndex(*model.pin_args())
    rng = np.random.default_rng(33)
    qrows = np.concatenate([[0, n0 - 1, 1500], rng.choice(n0, 10, replace=False), [n0 + 2, n0 + 60]])
    qs = np.ascontiguousarray(x[qrows])
    targets = np.concatenate([ids[rng.choice(n0, 500, replace=False)], ids[qrows[:13]], ids[:40], ids[n0 - 40:n0 + 65], [10 ** 8, -4]]).astype(np.int32)
    methods = (0, 1, 2) if with_vectors else (0,)
    spare = iter(np.arange(n0 + 200, ids.size))
    src = lambda n: np.array([next(spare) for _ in range(n)])

    def update(rows_ids, what, other_cell=False):
        rows_ids = np.asarray(rows_ids).reshape(-1)
        s = src(rows_ids.size)
        new_cell = t["coarse_id"][s].copy()
        if other_cell:
            r = np.searchsorted(model.ids, rows_ids)
            same = new_cell == model.cell[r]
            new_cell[same] = (new_cell[same] + 1) % model.cells
            assert (new_cell != model.cell[r]).all()
        a = _with_unknown(rows_ids, new_cell, t["codes"][s], take_v(s))
        got, exp = idx.update_rows(a[0], coarse_id=a[1], codes=a[2], vectors=a[3]), model.update(*a)
        assert got == exp == rows_ids.size and idx.N == model.N == idx.N, (what, got, exp)

    def check(what):
        tr._same_bytes(idx, gpu.IVPQIndex, model, what)
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

    def same_targets(what):
        got = idx.knn_join(qs, 5, targets, 3, 20, methods[-1], use_target_lists=True)
        exp, eit = oracle.ivpq_search_in(model.oracle_table(oracle), qs, 5, targets, 3, 20, methods[-1], use_target_lists=True)
        assert got[2] == eit, what
        util.assert_same_lists(got[0], got[1], exp, what)
        return exp["id"].copy()

    before = same_targets("before")
    update(ids[np.unique(qrows[:13])], "the queries' own rows to other cells: the first row, the last row, a middle row among them", other_cell=True)
    after = same_targets("the same targets after the cells changed")
    assert _ids_differ(before, after), "the update changed no list: the case does not bite"
    check("ivpq: the first, the last and eleven more rows in other cells")
    sl = np.arange(n0, n0 + 65)
    idx.append_rows(ids[sl], coarse_id=t["coarse_id"][sl], codes=t["codes"][sl], vectors=take_v(sl))
    model.append(ids[sl], t["coarse_id"][sl], t["codes"][sl], take_v(sl))
    cb2 = tm._nudged(model.codebook, 402)
    idx.update_codebook(cb2); model.update_codebook(cb2)
    update(np.concatenate([ids[n0 + 60:n0 + 65], model.ids[rng.choice(n0, 300, replace=False)]]), "appended rows and a tenth of the table after the swap")
    gone = np.concatenate([ids[n0 + 62:n0 + 64], ids[qrows[3:5]]])
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    for j in range(2):
        update(ids[700:701], f"the same row, call {j}")
    same_targets("the same targets after the second update")
    check("ivpq: appended rows updated after a swap, updated rows removed, one row twice")
    # refused: the answers, the footprint and the row count stay
    answers = lambda: [idx.knn_join(qs, 5, targets, 3, 20, method)[:2] for method in methods]
    was, nbytes, n_rows = answers(), idx.nbytes, idx.N
    two, s = ids[900:902], src(2)
    c2, k2, v2 = t["coarse_id"][s], t["codes"][s], take_v(s)
    high = k2.copy(); high[1, 0] = model.K
    refused = [((np.array([ids[900], ids[900]]), c2, k2, v2), rf"id {int(ids[900])} is listed twice, at positions 0 and 1"),
               ((np.array([ids[900], -7]), c2, k2, v2), r"id -7 at position 1"),
               ((two, [0, model.cells], k2, v2), rf"coarse_id {model.cells} of update row 1 "),
               ((two, c2, high, v2), rf"code {model.K} of update row 1 position 0 "),
               ((two, None, k2, v2), r"required"), ((two, c2, None, v2), r"required")]
    if with_vectors:
        refused.append(((two, c2, k2, None), r"required"))
    for args, words in refused:
        with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*" + words):
            idx.update_rows(args[0], coarse_id=args[1], codes=args[2], vectors=args[3])
        with pytest.raises(um.Refused):
            model.update(*args)
    gpu._check(idx.lib.freddy_gpu_update_rows(idx.h, 0, None, None, None, None, None))
    assert idx.update_rows(UNKNOWN, coarse_id=c2, codes=k2, vectors=v2) == model.update(UNKNOWN, c2, k2, v2) == 0
    assert idx.nbytes == nbytes and idx.N == model.N == n_rows
    for a, b in zip(was, answers()):
        tm._bits_equal(a, b, "ivpq: after the refused calls")
    idx.close()


# =======================================================================================
# 4. raw vectors
# =======================================================================================
def _vec_update(idx, model, ids, vectors, what):
    ids = np.asarray(ids).reshape(-1)
    a_ids, a_vec = _with_unknown(ids, vectors)
    got, exp = idx.update_rows(a_ids, vectors=a_vec), model.update(a_ids, a_vec)
    assert got == exp == ids.size and idx.N == model.N, (what, got, exp)


def _vec_k40(idx, oracle, model, qs, what):
    fresh = type(idx)(*model.pin_args())
    got = idx.search(qs, 40)
    tm._exact_same(got[0], got[1], [oracle.exact_knn(model.vectors, model.ids, q, 40) for q in qs], 40, what + " k=40")
    tm._bits_equal(got, fresh.search(qs, 40), what + " k=40")
    fresh.close()


@pytest.mark.parametrize("d", [300, 35])
def test_vec_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle, d):
    """8300 rows (just over 8192: the filter serves d = 300 by default; d = 35 has none).  Updated: the first row of a 32-row
    strip, lane 63 of a 64-row block, row N - 1 in the partial last block -- each a query's own row, replaced by a row from
    elsewhere -- then appended rows, one row twice, and removal of updated rows.  The footprint does not move across an update."""
    n0, total = 8300, 8400
    x, ids = tm._vec_table(d, total + 200)
    assert n0 % 64 != 0
    rng = np.random.default_rng(d + 1)
    qs, triples, sub = tm._vec_queries(x, ids, n0, total, rng)
    edges = np.array([32 * 7, 64 * 5 + 63, n0 - 1])
    qs = np.concatenate([x[edges], qs])
    triples[0, 0] = ids[edges[0]]; triples[3, 2] = ids[edges[2]]      # updated rows among the inputs of the analogies
    sub = np.concatenate([sub, ids[edges]]).astype(np.int32)
    model = um.VecModel(ids[:n0], x[:n0])
    idx = gpu.VectorIndex(*model.pin_args())
    nbytes = idx.nbytes
    spare = iter(np.arange(total, total + 200))
    src = lambda n: np.array([next(spare) for _ in range(n)])
    lists = lambda: np.stack([oracle.exact_knn(model.vectors, model.ids, q, 5)["id"] for q in qs[:3]])

    def check(what, more=False):
        names, _ = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, what, modes=(-1,))
        assert ("exact_filter" in names) == (d == 300), (what, sorted(names))
        if more:
            tr._vec_more(gpu, idx, model, qs, sub, what)
            _vec_k40(idx, oracle, model, qs, what)

    before = lists()
    assert all(ids[e] in row for e, row in zip(edges, before)), "a query's own row is not among its neighbours"
    _vec_update(idx, model, ids[edges], x[src(3)], "strip, block and table edges")
    assert _ids_differ(before, lists()), "the update changed no list: the case does not bite"
    assert idx.nbytes == nbytes, "the footprint moved across an update that leaves the filter's state as it was"
    check(f"vec d={d}: the first row of a strip, lane 63 of a block, the last row", more=True)
    idx.append_rows(ids[n0:total], vectors=x[n0:total]); model.append(ids[n0:total], x[n0:total])
    nbytes = idx.nbytes
    _vec_update(idx, model, np.concatenate([ids[n0:n0 + 40], ids[rng.choice(n0, 200, replace=False)]]), x[rng.choice(n0, 240, replace=False)], "appended rows and 200 more")
    for j in range(2):
        _vec_update(idx, model, ids[1000:1001], x[src(1)], f"the same row, call {j}")
    assert idx.nbytes == nbytes
    gone = np.concatenate([ids[n0:n0 + 10], ids[edges[:1]]])
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    check(f"vec d={d}: appended rows updated, one row twice, updated rows removed", more=True)
    # refused: the answers, the footprint and the row count stay
    answers = lambda: [idx.search(qs, 5), idx.search(qs, 5, subset_ids=sub)]
    was, nbytes, n_rows = answers(), idx.nbytes, idx.N
    for args, words in (((np.array([ids[50], ids[51], ids[50]]), x[:3]), rf"id {int(ids[50])} is listed twice, at positions 0 and 2"),
                        ((np.array([ids[50], -2]), x[:2]), r"id -2 at position 1"), ((ids[50:52], None), r"vectors are required")):
        with pytest.raises(gpu.FreddyGpuError, match=E_ARG + r".*" + words):
            idx.update_rows(args[0], vectors=args[1])
        with pytest.raises(um.Refused):
            model.update(*args)
    gpu._check(idx.lib.freddy_gpu_update_rows(idx.h, 0, None, None, None, None, None))
    assert idx.update_rows([4] + UNKNOWN, vectors=x[:3]) == model.update([4] + UNKNOWN, x[:3]) == 0
    assert idx.nbytes == nbytes and idx.N == model.N == n_rows
    for a, b in zip(was, answers()):
        tm._bits_equal(a, b, "vec: after the refused calls")
    idx.close()


def test_vec_the_scale_follows_the_largest_element_out_and_in(gpu, oracle):
    """One row 300 times as long as any other decides the power-of-two scale of the fragment copy.  Replaced by an ordinary row, the
    statistics are taken again over all rows: a fresh pin's scale and norm bound.  Then another row is replaced by a long one:
    the scale shrinks and every strip is laid out again.  Both with every row refined: no bracket violated.  The first two queries
    point along the two rows: each has its row among its neighbours before the update and, by the oracle's lists, not after."""
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n + 10)
    own = np.stack([x[4000], x[77]])                     # the directions of the two rows that will be replaced
    x[4000] *= np.float32(300.0)
    rng = np.random.default_rng(11)
    qs, triples, sub = tm._vec_queries(x, ids, 8000, n, rng)
    qs = np.ascontiguousarray(np.concatenate([own, qs]))
    lists = lambda: [oracle.exact_knn(model.vectors, model.ids, q, 5)["id"].tolist() for q in own]
    model = um.VecModel(ids[:n], x[:n])
    idx = gpu.VectorIndex(*model.pin_args())
    names, passes = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, "with the long row", modes=(-1,))
    assert "exact_filter" in names and passes > 0
    nbytes = idx.nbytes
    # (the long replacement points away from the row it replaces: with similarities that are dot products it leaves that query's list)
    for qi, (what, row, new) in enumerate((("the long row replaced by a small one", 4000, x[n + 1]),
                                           ("a row replaced by a longer one than any", 77, x[77] * np.float32(-500.0)))):
        before = lists()
        assert int(ids[row]) in before[qi], (what, "the row is not among its own query's neighbours: the case does not bite")
        _vec_update(idx, model, ids[row:row + 1], new[None], what)
        after = lists()
        assert int(ids[row]) not in after[qi] and before[qi] != after[qi], (what, "the update changed no list", before[qi], after[qi])
        assert idx.nbytes == nbytes, what
        idx.set_option("check_brackets", 0)
        names, passes = tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, what, modes=(-1,))
        assert "exact_filter" in names and passes > 0, (what, sorted(names))
        tr._vec_more(gpu, idx, model, qs, sub, what)
        idx.set_option("check_brackets", 4 | 8)
        checked = idx.bound_checked()
        tm._vec_check(gpu, oracle, idx, model, qs, triples, sub, what + ", every row refined", modes=(-1,))
        assert idx.bound_checked() - checked >= len(qs) * model.N and idx.bound_violations() == 0, what
    idx.close()


def test_vec_a_row_turns_non_finite_and_back(gpu, oracle):
    """A finite row turned NaN: the filter goes off (the all-exact kernels answer, as on a fresh pin of that table).  The only
    non-finite row turned finite again: the filter is back, with a fresh pin's kernels, bits and footprint."""
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n + 10)
    rng = np.random.default_rng(12)
    good = np.r_[0:123, 124:n]
    qs = np.ascontiguousarray(x[np.concatenate([[123], rng.choice(good, 10, replace=False)])])
    model = um.VecModel(ids[:n], x[:n])
    idx = gpu.VectorIndex(*model.pin_args())
    nbytes = idx.nbytes
    before = oracle.exact_knn(model.vectors, model.ids, qs[0], 5)["id"].copy()
    bad = x[123].copy(); bad[5] = np.float32(np.nan)

    def against_a_fresh_pin(what, filtered):
        fresh = gpu.VectorIndex(*model.pin_args())
        (gi, gs), names = tm._profiled(idx, lambda: idx.search(qs[1:], 5))
        (fi, fs), names_f = tm._profiled(fresh, lambda: fresh.search(qs[1:], 5))
        assert names == names_f and ("exact_filter" in names) == filtered and (filtered or "exact_scan" in names), (what, sorted(names), sorted(names_f))
        tm._bits_equal((gi, gs), (fi, fs), what)
        tn._exact_same(gi, gs, [oracle.exact_knn(model.vectors, model.ids, q, 5) for q in qs[1:]], 5, what)   # (every NaN as one)
        tm._bits_equal(idx.join(qs[1:], 5, ids[:n:3]), fresh.join(qs[1:], 5, ids[:n:3]), what + " join")
        assert idx.bound_violations() == 0
        out = fresh.nbytes
        fresh.close()
        return out

    against_a_fresh_pin("all rows finite", True)
    _vec_update(idx, model, ids[123:124], bad[None], "a row turns NaN")
    against_a_fresh_pin("one NaN row", False)
    _vec_update(idx, model, ids[123:124], x[n + 3][None], "the NaN row turns finite")
    assert against_a_fresh_pin("all rows finite again", True) == idx.nbytes == nbytes
    assert _ids_differ(before, oracle.exact_knn(model.vectors, model.ids, qs[0], 5)["id"])
    idx.close()


def test_vec_pinned_without_the_filter_stays_without_it(gpu, oracle, monkeypatch):
    d, n = 64, 8300
    x, ids = tm._vec_table(d, n + 10)
    monkeypatch.setenv("FREDDY_GPU_EXACT_FILTER", "0")
    model = um.VecModel(ids[:n], x[:n])
    idx = gpu.VectorIndex(*model.pin_args())
    monkeypatch.delenv("FREDDY_GPU_EXACT_FILTER")
    nbytes = idx.nbytes
    qs = np.ascontiguousarray(x[[3, 500, 8000]])
    before = np.stack([oracle.exact_knn(model.vectors, model.ids, q, 5)["id"] for q in qs])
    idx.set_option("exact_filter", 1)
    _vec_update(idx, model, ids[[3, 500]], x[n + 1:n + 3], "two rows")
    for mode in (1, -1):
        idx.set_option("exact_filter", mode)
        (gi, gs), names = tm._profiled(idx, lambda: idx.search(qs, 5))
        assert "exact_filter" not in names and "exact_scan" in names, (mode, sorted(names))
        tm._exact_same(gi, gs, [oracle.exact_knn(model.vectors, model.ids, q, 5) for q in qs], 5, f"pinned without the filter, option {mode}")
    after = np.stack([oracle.exact_knn(model.vectors, model.ids, q, 5)["id"] for q in qs])
    assert _ids_differ(before, after), "the update changed no list: the case does not bite"
    assert idx.nbytes == nbytes, "a fragment copy appeared"
    idx.close()


def test_ivfadc_search_pv_reads_the_updated_vectors(gpu, oracle):
    """Post verification of an ivf handle's lists against a vector handle, both updated for the same ids -- the queries' own rows,
    which get the codes, cells and vectors of rows elsewhere.  Before and after: the CPU model of tests/pv_model.py on the two
    models' tables (the oracle's search at k * pvf, exact_knn over its candidates), and afterwards the fresh pins' bits."""
    coarse, cb, ids, cell, codes, x = tm._ivf_source(300, 12, 256, 32)
    n0, k, pvf, W = 3000, 5, 10, 3
    imodel = um.IVFModel.from_rows(coarse, cb, ids[:n0], cell[:n0], codes[:n0])
    vmodel = um.VecModel(ids[:n0], x[:n0])
    ivf, vec = gpu.IVFIndex(*imodel.pin_args()), gpu.VectorIndex(*vmodel.pin_args())
    qrows = np.r_[20:36]
    qs = np.ascontiguousarray(x[qrows])

    def model_lists():
        lists = pm.ivf_lists(oracle, imodel.oracle_table(oracle), qs, k * pvf, W)
        return pm.expected(oracle, lists, vmodel.vectors, vmodel.ids, qs, k)[0]

    before = model_lists()
    got = ivf.search_pv(vec, qs, k, pvf, W)
    pm.same(got[0], got[1], before, k, "ivfadc_search_pv before the update")
    s = np.arange(n0 + 100, n0 + 100 + qrows.size)
    _ivf_update(ivf, imodel, ids[qrows], cell[s], codes[s], "pv: codes")
    _vec_update(vec, vmodel, ids[qrows], x[s], "pv: vectors")
    after = model_lists()
    assert [e["id"].tolist() for e in before] != [e["id"].tolist() for e in after], "the update changed no list: the case does not bite"
    f_ivf, f_vec = gpu.IVFIndex(*imodel.pin_args()), gpu.VectorIndex(*vmodel.pin_args())
    got = ivf.search_pv(vec, qs, k, pvf, W)
    pm.same(got[0], got[1], after, k, "ivfadc_search_pv after the update")
    tm._bits_equal(got, f_ivf.search_pv(f_vec, qs, k, pvf, W), "ivfadc_search_pv after the update")
    # an update of the vectors alone: the same candidates, re-ranked against the new rows
    _vec_update(vec, vmodel, ids[40:44], x[s[:4]], "pv: vectors only")
    got = ivf.search_pv(vec, qs, k, pvf, W)
    pm.same(got[0], got[1], model_lists(), k, "ivfadc_search_pv after an update of the vectors alone")
    for h in (ivf, vec, f_ivf, f_vec):
        h.close()


# =======================================================================================
# 5. the host mirror
# =======================================================================================
def _session(ids, x, pq, ivf, iv):
    from freddy_amd import udf
    s = udf.Session()
    s.load_vecs_norm(ids, x)
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    s.load_ivfadc(ivf["coarse"], ivf["codebook"], ivf["ids"], ivf["cell"], ivf["codes"])
    s.load_ivpq(iv["codebook"], iv["coarse"], iv["ids"], iv["coarse_id"], iv["codes"], iv["stats"])
    return s


def test_update_rows_equals_a_session_loaded_from_the_updated_tables(gpu):
    """update_rows on a session with every table loaded and the vector handle pinned; then a handful of UDFs answer as a session
    loaded from the tables with those rows replaced (their codes and cells quantised against the same codebooks), and a
    following insert_batch and delete_rows work on both alike."""
    N = 20000
    x = util.corpus(N).numpy().copy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    pq, ivf0, iv = dict(util.pq_tables(N=N, K=256)), util.ivf_tables(N=N, C=32, K=256), dict(util.ivpq_tables(N=N))
    ivf = {k: ivf0[k] for k in ("coarse", "codebook", "ids", "codes")}
    ivf["cell"] = np.repeat(np.arange(32), np.diff(ivf0["list_off"])).astype(np.int32)
    a = _session(ids, x, pq, ivf, iv)
    qrows = np.array([123, 4000, 77])
    a.k_nearest_neighbour(x[123], 3)                     # google_vecs_norm is pinned before the rows change
    rng = np.random.default_rng(13)
    upd = np.concatenate([ids[qrows], ids[rng.choice(N, 300, replace=False)], [N]]).astype(np.int32)
    upd = np.unique(upd)[rng.permutation(np.unique(upd).size)]
    new = x[rng.choice(N, upd.size, replace=False)] * np.float32(0.999)
    before = [a.k_nearest_neighbour(x[r], 5)["id"].tolist() for r in qrows]
    ask_ids, ask_vec = np.concatenate([upd, [N + 5]]).astype(np.int32), np.concatenate([new, new[:1]])
    assert a.update_rows(ask_ids, ask_vec) == upd.size
    # the model's tables: the same quantisation against the same codebooks, the multi-index cell by insert_batch's formula
    qz = gpu.insert_quantize(new, pq_codebook=pq["codebook"], residual_codebook=ivf["codebook"], coarse=ivf["coarse"],
                             ivpq_codebook=iv["codebook"], coarse_multi=iv["coarse"])
    x2 = x.copy(); x2[upd - 1] = new
    positions = iv["coarse"].shape[0]
    multi = (qz["coarse_multi_codes"].astype(np.int64) * positions ** np.arange(positions)).sum(axis=1).astype(np.int32)
    pq2, ivf2, iv2 = dict(pq), dict(ivf), dict(iv)
    for t, fields in ((pq2, {"codes": qz["pq_codes"]}), (ivf2, {"codes": qz["residual_codes"], "cell": qz["coarse_id"]}),
                      (iv2, {"codes": qz["ivpq_codes"], "coarse_id": multi})):
        rows = {int(i): r for r, i in enumerate(t["ids"].tolist())}
        at = np.array([rows[int(i)] for i in upd])
        for name, val in fields.items():
            t[name] = np.array(t[name], copy=True)
            t[name][at] = val
    b = _session(ids, x2, pq2, ivf2, iv2)
    targets = np.concatenate([ids[::13], upd[:50]]).astype(np.int32)
    three = np.arange(1, 4, dtype=np.int32)
    draws = np.random.default_rng(14).random(64)

    def same(what):
        for r in qrows:
            for name, call in (("k_nearest_neighbour", lambda s: s.k_nearest_neighbour(x[r], 5)), ("pq_search", lambda s: s.pq_search(x[r], 6)),
                               ("ivfadc_search", lambda s: s.ivfadc_search(x[r], 6))):
                assert call(a).tobytes() == call(b).tobytes(), (what, name, r)
        assert a.knn_join(x[qrows], three, 4, targets).tobytes() == b.knn_join(x[qrows], three, 4, targets).tobytes(), (what, "knn_join")
        assert a.analogy_3cosadd(int(upd[40]), int(ids[10]), int(ids[20])) == b.analogy_3cosadd(int(upd[40]), int(ids[10]), int(ids[20])), (what, "analogy_3cosadd")
        tokens = np.unique(np.concatenate([upd[30:70], ids[500:560]])).astype(np.int32)   # (updated rows that stay to the end)
        assert np.array_equal(a.cluster_exact(tokens, 4, draws), b.cluster_exact(tokens, 4, draws)), (what, "cluster_exact")

    same("after update_rows")
    assert before != [a.k_nearest_neighbour(x[r], 5)["id"].tolist() for r in qrows], "the update changed no list: the case does not bite"
    v = x[rng.choice(N, 9, replace=False)] * np.float32(0.998)
    na, nb = a.insert_batch(v), b.insert_batch(v)
    assert na.tolist() == nb.tolist() == list(range(N + 1, N + 10))
    gone = np.concatenate([upd[:30], na[:2]]).astype(np.int32)
    assert a.delete_rows(gone) == b.delete_rows(gone) == gone.size
    same("after insert_batch and delete_rows")
    a.close(); b.close()
