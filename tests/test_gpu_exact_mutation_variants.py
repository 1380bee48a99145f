"""-m gpu: update_rows, append_rows and remove_rows on vector handles under options exact_wide and exact_filter_k.  The statistics
and the fragment-order copy of a wide table are the option's state (csrc/exact_wide.hip): exf_table_stats picks its shape rule
from the option, update_rows reaches it with a changed_strips list whose strips are T * 2 KiB long at the WIDE T, remove_rows
takes the statistics again from row 0, exact_wide = 0 releases the copy.  tests/update_model.py's VecModel applies every step to
host arrays; after every step the handle is compared with the oracle on the model's table and with a FRESH pin of it that has the
same options set: ids, similarity bits, the kernels that served the call, freddy_gpu_index_bytes.  Nothing has a tolerance."""
import numpy as np
import pytest

import test_gpu_mutation as tm
import test_gpu_nonfinite as tn
import update_model as um
from test_gpu_update import _ids_differ, _vec_update

pytestmark = pytest.mark.gpu
WIDE = (("exact_wide", 1),)
WIDE_K = (("exact_wide", 1), ("exact_filter_k", 1024))
NARROW_K = (("exact_filter_k", 1024),)


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _set(idx, options):
    for name, value in options:
        idx.set_option(name, value)
    return idx


def _path(names, d, k, filtered):
    if not filtered:
        return "exact_scan" in names and "exact_filter" not in names and "exact_filter_wide" not in names
    want = {"exact_filter_wide" if d > 512 else "exact_filter", "exact_refine", "exact_threshold_rank" if k > 32 else "exact_threshold"}
    return want <= names and "exact_scan" not in names


def _check(gpu, oracle, idx, model, options, qs, ks, what, filtered=True, by_id=None, appended=False, footprint=True, removed_from=None):
    """search at every k (and exact_search_ids over the rows `by_id`): the oracle's lists, a fresh pin's bits, kernels and nbytes.
    appended: the fragment copy has grown in place -- the footprint lies in the window tests/test_gpu_mutation.py derives for it,
    fresh - (need / 8 + 256) <= mutated <= fresh, need the bytes of the copy.  footprint = False: while a row of the handle is
    not finite it keeps the copy a fresh pin of that table never builds (as tests/test_gpu_update.py has it for narrow tables).
    removed_from: the footprint before rows were removed -- the buffers stay, so the handle lies between a fresh pin and that
    (tests/test_gpu_removal.py)."""
    fresh = _set(gpu.VectorIndex(*model.pin_args()), options)
    d = model.vectors.shape[1]
    for k in ks:
        w = f"{what} k={k}"
        got, names = tm._profiled(idx, lambda: idx.search(qs, k))
        fgot, fnames = tm._profiled(fresh, lambda: fresh.search(qs, k))
        tn._exact_same(got[0], got[1], [oracle.exact_knn(model.vectors, model.ids, q, k) for q in qs], k, w)      # (every NaN as one)
        tm._bits_equal(got, fgot, w)
        assert names == fnames and _path(names, d, k, filtered), (w, sorted(names), sorted(fnames))
        if by_id is not None:
            qids = model.ids[by_id]
            (qi, gi, gs), names = tm._profiled(idx, lambda: idx.exact_search_ids(qids, k))
            (_, fi, fs), fnames = tm._profiled(fresh, lambda: fresh.exact_search_ids(qids, k))
            assert qi.tolist() == qids.tolist(), w
            tn._exact_same(gi, gs, [oracle.exact_knn(model.vectors, model.ids, model.vectors[r], k) for r in by_id], k, w + " by id")
            tm._bits_equal((gi, gs), (fi, fs), w + " by id")
            assert names == fnames and _path(names, d, k, filtered), (w + " by id", sorted(names), sorted(fnames))
    need = ((model.N + 31) // 32) * ((d + 15) // 16) * 2 * 64 * 16
    slack = need // 8 + 256 if appended else 0
    assert not footprint or fresh.nbytes - slack <= idx.nbytes <= (removed_from or fresh.nbytes), (what, "the footprint differs from a fresh pin's", idx.nbytes, fresh.nbytes, slack)
    assert idx.bound_violations() == 0 and fresh.bound_violations() == 0, what
    fresh.close()


def test_wide_sequence_equals_oracle_and_a_fresh_pin(gpu, oracle):
    """d = 768, 8300 rows, exact_wide = 1: tests/test_gpu_update.py's vector sequence.  Updated: the first row of a 32-row strip,
    lane 63 of a 64-row block, the last row -- each a query's own row -- then appended rows, one row twice, updated rows removed.
    By-id queries (gathered on the device) at k = 5 and k = 100 before and after."""
    d, n0, total = 768, 8300, 8400
    x, ids = tm._vec_table(d, total + 200)
    rng = np.random.default_rng(d + 1)
    edges = np.array([32 * 7, 64 * 5 + 63, n0 - 1])
    qs = np.concatenate([x[edges], x[rng.choice(n0, 6, replace=False)], x[n0 + 3:n0 + 5]])
    by_id = np.array([32 * 7, 64 * 5 + 63, 5000])       # (ascending: exact_search_ids answers in table order)
    model = um.VecModel(ids[:n0], x[:n0])
    idx = _set(gpu.VectorIndex(*model.pin_args()), WIDE_K)
    spare = iter(np.arange(total, total + 200))
    src = lambda n: np.array([next(spare) for _ in range(n)])
    lists = lambda: np.stack([oracle.exact_knn(model.vectors, model.ids, q, 5)["id"] for q in qs[:3]])
    _check(gpu, oracle, idx, model, WIDE_K, qs, (5, 100), "wide: as pinned", by_id=by_id)
    nbytes, before = idx.nbytes, lists()
    assert all(ids[e] in row for e, row in zip(edges, before)), "a query's own row is not among its neighbours"
    _vec_update(idx, model, ids[edges], x[src(3)], "strip, block and table edges")
    assert _ids_differ(before, lists()), "the update changed no list: the case does not bite"
    assert idx.nbytes == nbytes, "the footprint moved across an update that leaves the scale as it was"
    _check(gpu, oracle, idx, model, WIDE_K, qs, (5, 100), "wide: the first row of a strip, lane 63 of a block, the last row", by_id=by_id)
    idx.append_rows(ids[n0:total], vectors=x[n0:total]); model.append(ids[n0:total], x[n0:total])
    nbytes = idx.nbytes
    _vec_update(idx, model, np.concatenate([ids[n0:n0 + 40], ids[rng.choice(n0, 200, replace=False)]]), x[rng.choice(n0, 240, replace=False)], "appended rows and 200 more")
    for j in range(2):
        _vec_update(idx, model, ids[1000:1001], x[src(1)], f"the same row, call {j}")
    assert idx.nbytes == nbytes
    _check(gpu, oracle, idx, model, WIDE_K, qs, (5, 100), "wide: appended rows updated, one row twice", appended=True)
    gone = np.concatenate([ids[n0:n0 + 10], ids[edges[:1]]])
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    _check(gpu, oracle, idx, model, WIDE_K, qs, (5, 100), "wide: updated rows removed", by_id=np.array([32 * 7, 64 * 5 + 62, 5000]), appended=True,
           removed_from=nbytes)
    idx.close()


def test_wide_scale_follows_the_largest_element_out_and_in(gpu, oracle):
    """One row 300 times as long as any other decides the scale of the wide copy; replaced by an ordinary row the statistics are
    taken again over all rows, then another row becomes the longest and every strip is laid out again.  Every row refined: no
    bracket violated, Q N rows checked."""
    d, n = 768, 8300
    x, ids = tm._vec_table(d, n + 10)
    own = np.stack([x[4000], x[77]])
    x[4000] *= np.float32(300.0)
    qs = np.ascontiguousarray(np.concatenate([own, x[np.random.default_rng(11).choice(8000, 8, replace=False)]]))
    lists = lambda: [oracle.exact_knn(model.vectors, model.ids, q, 5)["id"].tolist() for q in own]
    model = um.VecModel(ids[:n], x[:n])
    idx = _set(gpu.VectorIndex(*model.pin_args()), WIDE)
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: with the long row")
    nbytes = idx.nbytes
    for qi, (what, row, new) in enumerate((("wide: the long row replaced by a small one", 4000, x[n + 1]),
                                           ("wide: a row replaced by a longer one than any", 77, x[77] * np.float32(-500.0)))):
        before = lists()
        assert int(ids[row]) in before[qi], (what, "the row is not among its own query's neighbours: the case does not bite")
        _vec_update(idx, model, ids[row:row + 1], new[None], what)
        assert int(ids[row]) not in lists()[qi], (what, "the update changed no list")
        assert idx.nbytes == nbytes, what
        _check(gpu, oracle, idx, model, WIDE, qs, (5, 32), what)
        checked = idx.bound_checked()
        _check(gpu, oracle, idx, model, WIDE + (("check_brackets", 4),), qs, (5,), what + ", every row refined")
        idx.set_option("check_brackets", 4)
        _check(gpu, oracle, idx, model, WIDE + (("check_brackets", 4),), qs, (5,), what + ", every row refined")
        assert idx.bound_checked() - checked == len(qs) * model.N and idx.bound_violations() == 0, what
        idx.set_option("check_brackets", 0)
    idx.close()


def test_wide_row_turns_non_finite_and_back_and_the_option_around_mutations(gpu, oracle):
    d, n = 768, 8300
    x, ids = tm._vec_table(d, n + 10)
    rng = np.random.default_rng(12)
    qs = np.ascontiguousarray(x[rng.choice(np.r_[0:123, 124:n], 10, replace=False)])
    model = um.VecModel(ids[:n], x[:n])
    plain = gpu.VectorIndex(*model.pin_args())
    without = plain.nbytes
    idx = _set(plain, WIDE)
    nbytes = idx.nbytes
    assert nbytes - without >= n * d * 4
    bad = x[123].copy(); bad[5] = np.float32(np.nan)
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: all rows finite")
    _vec_update(idx, model, ids[123:124], bad[None], "a row turns NaN")
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: one NaN row", filtered=False, footprint=False)     # (a fresh pin that accepts the option over a NaN row)
    _vec_update(idx, model, ids[123:124], x[n + 3][None], "the NaN row turns finite")
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: all rows finite again")
    assert idx.nbytes == nbytes
    # exact_wide 1 -> 0 -> 1 around a mutation: the copy is released and rebuilt from the mutated rows
    idx.set_option("exact_wide", 0)
    assert idx.nbytes == without
    before = oracle.exact_knn(model.vectors, model.ids, qs[0], 5)["id"].copy()
    _vec_update(idx, model, before[:2], x[n + 4:n + 6], "two of query 0's neighbours, the option off")
    assert _ids_differ(before, oracle.exact_knn(model.vectors, model.ids, qs[0], 5)["id"])
    _check(gpu, oracle, idx, model, (("exact_wide", 0),), qs, (5,), "wide: the option off", filtered=False)
    idx.set_option("exact_wide", 1)
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: the option on again after an update")
    assert idx.nbytes == nbytes
    # rows removed down below 8192: auto takes the scan, forced takes the wide filter
    gone = model.ids[200:400].copy()
    assert idx.remove_rows(gone) == model.remove(gone) == 200 and model.N < 8192
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "wide: 8100 rows, exact_filter = -1", filtered=False, removed_from=nbytes)
    idx.set_option("exact_filter", 1)
    _check(gpu, oracle, idx, model, WIDE + (("exact_filter", 1),), qs, (5,), "wide: 8100 rows, exact_filter = 1", removed_from=nbytes)
    idx.close()


def test_narrow_mutations_before_a_search_at_k_above_32(gpu, oracle):
    """d = 300, exact_filter_k = 1024: an update, a remove and an append, each followed by searches at k = 100 and k = 1024.  One
    row of every search's own top-k is an updated row: by the oracle the lists changed."""
    d, n0, total = 300, 8300, 8400
    x, ids = tm._vec_table(d, total + 50)
    qs = np.ascontiguousarray(x[[32 * 7, 64 * 5 + 63, n0 - 1, 4000]])
    by_id = np.array([32 * 7, 4001])
    model = um.VecModel(ids[:n0], x[:n0])
    idx = _set(gpu.VectorIndex(*model.pin_args()), NARROW_K)
    lists = lambda k: np.stack([oracle.exact_knn(model.vectors, model.ids, q, k)["id"] for q in qs])
    _check(gpu, oracle, idx, model, NARROW_K, qs, (100, 1024), "narrow: as pinned", by_id=by_id)
    before = {k: lists(k) for k in (100, 1024)}
    rows = np.unique(np.concatenate([before[100][:, 0], before[100][:, 50], before[1024][:, 99]]))     # ids in every query's top 100
    _vec_update(idx, model, rows, -x[total:total + rows.size], "rows of every query's top 100")
    after = {k: lists(k) for k in (100, 1024)}
    assert all((before[k][qi] != after[k][qi]).any() for k in (100, 1024) for qi in range(len(qs))), "an update changed no list: the case does not bite"
    _check(gpu, oracle, idx, model, NARROW_K, qs, (100, 1024), "narrow: after the update", by_id=by_id)
    nbytes = idx.nbytes
    gone = after[100][:, 1].copy()
    assert idx.remove_rows(gone) == model.remove(gone) == np.unique(gone).size
    _check(gpu, oracle, idx, model, NARROW_K, qs, (100, 1024), "narrow: after the remove", removed_from=nbytes)
    idx.append_rows(ids[n0:total], vectors=x[n0:total]); model.append(ids[n0:total], x[n0:total])
    _check(gpu, oracle, idx, model, NARROW_K, qs, (100, 1024), "narrow: after the append", by_id=by_id, appended=True)
    idx.close()


def test_exact_wide_set_on_a_table_that_holds_a_nan_row(gpu, oracle):
    """the option is accepted, the all-exact scan answers; the row rewritten finite, the wide filter serves with a fresh pin's footprint"""
    d, n = 768, 8300
    x, ids = tm._vec_table(d, n + 2)
    x[123, 5] = np.float32(np.nan)
    qs = np.ascontiguousarray(x[[7, 4000, 8000]])
    model = um.VecModel(ids[:n], x[:n])
    idx = _set(gpu.VectorIndex(*model.pin_args()), WIDE)
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "exact_wide = 1 over a NaN row", filtered=False)
    _vec_update(idx, model, ids[123:124], x[n:n + 1], "the NaN row turns finite")
    _check(gpu, oracle, idx, model, WIDE, qs, (5,), "exact_wide = 1, the NaN row rewritten")
    idx.close()
