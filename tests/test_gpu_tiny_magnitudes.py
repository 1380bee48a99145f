"""-m gpu: the small end of binary32 (tests/tiny_inputs.py; tests/test_tiny_inputs_cpu.py proves the cases).  Everything is bit
for bit against the oracle or the numpy models; there is no tolerance anywhere.

a. The exact filter family.  Cosine similarity is bilinear, so a table at 2^-80 has similarities that are normal numbers while the
   squares of its elements are 0: a bracket eps(q) = EXF_EPS X |q| whose X or |q| came from a binary32 sum of squares alone has no
   width there (csrc/exact2.h, "Small magnitudes").  Every case runs with the filter forced (exact_filter = 1), with every row
   refined and compared with its bracket (check_brackets = 4: zero violations, Q N rows checked) and without; the profile must
   name the filter's kernels and not the all-exact scan: the filter is switched off in NO case.  The near-tie cluster of the
   inputs makes a bracket that is too narrow show in the lists too (query 0).
b. (tests/test_gpu_table_split.py: the quadratic brackets at 2^-64, 2^-80 and 2^-140.)
c. The chains that divide and take square roots (tokenize, the post verification, the approximate analogies) and the plain chains
   (similarity by id, assign) over tables at 2^-64, 2^-70 (sums of squares subnormal), 2^-80 (the sum is 0: inf / NaN as the
   reference produces them) and 2^-120 (centroid quotients in the subnormals), at d = 32 and d = 25 (the scalar loads).

Observed on an MI355X before exf_table_stats_kernel / exf_prep_kernel bounded the norms from the largest |element| where the
squares underflow (rows outside their bracket in one search of 70 x 2 080 pairs / in the join of 6 930): squares_vanish_80
119 460 / 5 688, squares_vanish_100 37 757 / 1 711, tiny_query 119 460 / 5 688, mixed 113 762 / 5 467, unscale_underflows (the
unscale factor 2^-(eq + ex) is 0) 4 743 / 238; the other cases passed, squares_rounded_away_74 because some rows keep two
subnormal ulps in the maximum, which happens to be about the true norm.  The lists equalled the oracle's in all of them, the
near-tie cluster included: at d = 32 the threshold's two roundings down by 2.4e-7 happen to cover the chain's few ulps
(DESIGN.md 5.6).  Section c exposed nothing."""
import functools

import numpy as np
import pytest

import analogy_model as am
import assign_model as asm
import similarity_model as sm
import tiny_inputs as ti
import tokenize_model as tm

pytestmark = pytest.mark.gpu
U = np.uint32
KS = (1, 5, 32)
N_TARGETS, N_QIDS, N_TRIPLES = 100, 70, 40
ALL_EXACT = {"exact_scan", "exact_merge", "analogy_scan", "analogy_merge"}


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


def _lists(entries, k):
    """the oracle's entries (at least k per query here) as (ids[Q][k], similarities[Q][k])"""
    return np.stack([e["id"][:k] for e in entries]).astype(np.int32), np.stack([e["dist"][:k] for e in entries]).astype(np.float32)


def _same(got, exp, what):
    gi, gs = got[-2], got[-1]
    bad = np.flatnonzero((gi != exp[0]).any(1))
    assert bad.size == 0, (what, "ids differ for queries", bad[:8].tolist(), gi[bad[0]].tolist(), exp[0][bad[0]].tolist())
    bad = np.flatnonzero((gs.view(U) != exp[1].view(U)).any(1))
    assert bad.size == 0, (what, "similarity bits differ for queries", bad[:8].tolist())


def _sets():
    """(target ids of the joins, the rows whose ids are the queries of the by-id and by-text calls -- cluster rows among them)"""
    ids, _, _ = ti.base()
    rng = np.random.default_rng(5)
    targets = np.sort(ids[np.concatenate([rng.choice(ti.N, size=N_TARGETS - 20, replace=False), np.arange(110, 130)])])
    targets = np.unique(targets)
    qrows = np.unique(np.concatenate([rng.choice(ti.N, size=N_QIDS - 10, replace=False), np.arange(100, 110)]))
    return targets, qrows


@functools.lru_cache(maxsize=None)
def _expected(oracle, name):
    """the oracle's lists of a case, computed once and shared"""
    ids, t, q = ti.case(name)
    targets, qrows = _sets()
    return dict(knn=[oracle.exact_knn(t, ids, v, 32) for v in q],
                join=[oracle.exact_knn(t, ids, v, 5, targets) for v in q],
                ids_knn=[oracle.exact_knn(t, ids, t[r], 5) for r in qrows],
                ids_join=[oracle.exact_knn(t, ids, t[r], 5, targets) for r in qrows])


def _pin(gpu, ids, t, check_brackets=0, exact_filter=1):
    idx = gpu.VectorIndex(ids, t)
    idx.set_option("exact_filter", exact_filter)
    idx.set_option("check_brackets", check_brackets)
    return idx


# ---- a. the exact filter family -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ti.CASES))
def test_exact_knn_lists_and_brackets(gpu, oracle, name):
    """search at k = 1, 5, 32 with every row refined and without: the oracle's ids and similarity bits, the filter's kernels, no
    bracket left, Q N rows checked.  At k = 5 the all-exact kernels (exact_filter = 0, a handle of its own) give the same lists."""
    ids, t, q = ti.case(name)
    exp = _expected(oracle, name)
    idx = _pin(gpu, ids, t)
    for brackets in (4, 0):
        idx.set_option("check_brackets", brackets)
        for k in KS:
            what = f"{name} check_brackets {brackets} k {k}"
            v0, c0 = idx.bound_violations(), idx.bound_checked()
            got, names = _profiled(idx, lambda: idx.search(q, k))
            viol, checked = idx.bound_violations() - v0, idx.bound_checked() - c0
            print(what, "violations", viol, "checked", checked, "lists equal", bool(np.array_equal(got[0], _lists(exp["knn"], k)[0])))
            assert {"exact_filter", "exact_refine"} <= names and not (names & ALL_EXACT), (what, sorted(names))
            assert viol == 0, (what, "rows outside their bracket", viol)
            assert checked == (ti.Q * ti.N if brackets else 0), (what, checked)
            _same(got, _lists(exp["knn"], k), what)
    idx.close()
    plain = _pin(gpu, ids, t, exact_filter=0)
    got, names = _profiled(plain, lambda: plain.search(q, 5))
    assert "exact_scan" in names and "exact_filter" not in names, sorted(names)
    _same(got, _lists(exp["knn"], 5), f"{name} all-exact kernels")
    plain.close()


@pytest.mark.parametrize("name", sorted(ti.CASES))
def test_join_by_id_and_by_text_lists_and_brackets(gpu, oracle, name):
    """The same cases once each through join, exact_search_ids, exact_join_ids and exact_search_texts (one token per text, not
    normalised: the text vector is the row).  The queries of the by-id and by-text calls are table rows: both sides are small."""
    ids, t, q = ti.case(name)
    exp = _expected(oracle, name)
    targets, qrows = _sets()
    qids = ids[qrows]
    idx = _pin(gpu, ids, t, check_brackets=4)
    calls = [
        ("join", lambda: idx.join(q, 5, targets), exp["join"], "exact_join", ti.Q * targets.size),
        ("exact_search_ids", lambda: idx.exact_search_ids(qids, 5), exp["ids_knn"], "exact", qrows.size * ti.N),
        ("exact_join_ids", lambda: idx.exact_join_ids(qids, 5, targets), exp["ids_join"], "exact_join", qrows.size * targets.size),
        ("exact_search_texts", lambda: idx.search_texts([[i] for i in qids], 5, normalize=False), exp["ids_knn"], "exact", qrows.size * ti.N),
    ]
    for call_name, call, entries, prefix, n_checked in calls:
        what = f"{name} {call_name}"
        v0, c0 = idx.bound_violations(), idx.bound_checked()
        got, names = _profiled(idx, call)
        viol, checked = idx.bound_violations() - v0, idx.bound_checked() - c0
        print(what, "violations", viol, "checked", checked)
        assert {prefix + "_filter", prefix + "_refine"} <= names and not (names & ALL_EXACT), (what, sorted(names))
        assert viol == 0 and checked == n_checked, (what, viol, checked)
        if call_name.endswith("_ids"):
            assert np.array_equal(got[0], qids), what
        if call_name == "exact_search_texts":
            assert np.all(got[0] == 1), what
        _same(got, _lists(entries, 5), what)
    assert idx.last_join_stats()["redone_queries"] == 0
    idx.close()


@pytest.mark.parametrize("exp2", [0, -70, -80])
def test_exact_analogies_over_small_tables(gpu, exp2):
    """3CosAdd and 3CosMul, k = 5, every row refined (check_brackets = 8), 40 triples (a pass of 32 and one of 8) against the numpy
    model; the unit table is the control."""
    ids, _, _ = ti.base()
    t = ti.scaled_table(exp2)
    rng = np.random.default_rng(17)
    triples = ids[rng.integers(0, ti.N, size=(N_TRIPLES, 3))]
    x_t = np.ascontiguousarray(t.T)
    idx = _pin(gpu, ids, t, check_brackets=8)
    for method in ("3cosadd", "3cosmul"):
        what = f"table x 2^{exp2} {method}"
        with np.errstate(all="ignore"):
            ei, es = am.model(t, ids, triples, 5, method, x_t=x_t)
        v0, c0 = idx.bound_violations(), idx.bound_checked()
        (gi, gs), names = _profiled(idx, lambda: idx.analogy(triples, k=5, method=method))
        viol, checked = idx.bound_violations() - v0, idx.bound_checked() - c0
        print(what, "violations", viol, "checked", checked, sorted(names))
        assert {"analogy_filter", "analogy_refine"} <= names and not (names & ALL_EXACT), (what, sorted(names))
        assert viol == 0 and checked > 0, (what, viol, checked)
        assert np.array_equal(gi, ei), (what, np.flatnonzero((gi != ei).any(1))[:8].tolist())
        assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)), (what, np.flatnonzero((gs.view(np.uint64) != es.view(np.uint64)).any(1))[:8].tolist())
    idx.close()


@pytest.mark.parametrize("name", ["squares_vanish_80", "mixed"])
def test_mutated_handle_brackets_equal_a_fresh_pin(gpu, oracle, name):
    """The norm bound folds over appended slices as it does over a whole table: a handle pinned on the first 1 000 rows (in `mixed`
    all of them unit rows) and extended by the rest, then with 40 rows rewritten and written back, then with 40 rows removed, gives
    a fresh pin's lists, refines as many candidates as the fresh pin in the join, and leaves no bracket."""
    ids, t, q = ti.case(name)
    targets, _ = _sets()
    idx = _pin(gpu, ids[:1000], t[:1000], check_brackets=4)
    idx.append_rows(ids[1000:], vectors=t[1000:])
    fresh = _pin(gpu, ids, t, check_brackets=4)
    exp = _expected(oracle, name)
    for h in (idx, fresh):
        _same(h.search(q, 5), _lists(exp["knn"], 5), name)
    for brackets in (4, 0):
        for h in (idx, fresh):
            h.set_option("check_brackets", brackets)
            _same(h.join(q, 5, targets), _lists(exp["join"], 5), name)
        assert idx.last_join_stats() == fresh.last_join_stats(), (name, brackets)
    # update_rows: 40 rows become unit-scale rows (X grows by 2^80 where the table was small) and go back: a fresh pin's lists and
    # candidate counts both times, every bracket checked
    _, unit, _ = ti.base()
    rows = np.arange(1040, 1080)           # (rows x 2^-80 in both cases)
    changed = np.array(t)
    changed[rows] = unit[rows]
    for table in (changed, t):
        assert idx.update_rows(ids[rows], vectors=table[rows]) == rows.size
        again = _pin(gpu, ids, table, check_brackets=4)
        for h in (idx, again):
            h.set_option("check_brackets", 4)
        a, b = idx.search(q, 5), again.search(q, 5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(U), b[1].view(U)), name
        for brackets in (4, 0):
            for h in (idx, again):
                h.set_option("check_brackets", brackets)
            a, b = idx.join(q, 5, targets), again.join(q, 5, targets)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(U), b[1].view(U)), name
            assert idx.last_join_stats() == again.last_join_stats(), (name, brackets)
        assert again.bound_violations() == 0, name
        again.close()
    gone = ids[1500:1540]
    keep = np.ones(ti.N, bool)
    keep[1500:1540] = False
    idx.remove_rows(gone)
    fresh2 = _pin(gpu, ids[keep], t[keep])
    a, b = idx.search(q, 32), fresh2.search(q, 32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(U), b[1].view(U)), name
    assert idx.bound_violations() == 0 and fresh.bound_violations() == 0 and fresh2.bound_violations() == 0
    for h in (idx, fresh, fresh2):
        h.close()


# ---- c. chains that divide and take square roots, and the plain chains, over small tables ---------------------------------------
N_C = 600
C_EXPS = (-64, -70, -80)
IVF_SHAPE = {32: 4, 25: 5}       # d -> m


@functools.lru_cache(maxsize=None)
def _small(d, exp2):
    """(ids 1 .. N_C as the index builders number rows, the first N_C rows / d columns of the base table x 2^exp2)"""
    return np.arange(1, N_C + 1, dtype=np.int32), ti.scaled_table(exp2, d=d, n=N_C)


def _same_floats(got, exp, what):
    """bit for bit; a NaN is any NaN"""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    gn, en = np.isnan(got), np.isnan(exp)
    assert got.shape == exp.shape and np.array_equal(gn, en), (what, "NaNs sit elsewhere")
    bad = np.argwhere(got.view(U)[~gn] != exp.view(U)[~en])
    assert bad.size == 0, (what, "bits differ", bad[:5].tolist())


def _sums_of_squares(t):
    with np.errstate(all="ignore"):
        return sm.chain(t, t)


@pytest.mark.parametrize("exp2", C_EXPS)
@pytest.mark.parametrize("d", sorted(IVF_SHAPE))
def test_similarity_and_assign_over_small_tables(gpu, d, exp2):
    ids, t = _small(d, exp2)
    sq = _sums_of_squares(t)
    assert (sq.max() == 0) if exp2 == -80 else (0 < sq.max() < 2.0 ** -126), (exp2, sq.max())     # the table is what section c says
    rng = np.random.default_rng(100 + d)
    a, b = rng.choice(ids, 200).astype(np.int32), rng.choice(ids, 200).astype(np.int32)
    a[7], b[11] = N_C + 50, -3                                                                     # ids without a row
    vec = gpu.VectorIndex(ids, t)
    what = f"d {d} table x 2^{exp2}"
    gs, gk = vec.similarity_pairs(a, b)
    es, ek = sm.pairs(ids, t, a, b)
    assert np.array_equal(gk, ek), what
    _same_floats(gs, es, what + " pairs")
    for a_side in (a[:40], np.ascontiguousarray(rng.standard_normal((40, d)), np.float32)):
        go, gka, gkb = vec.similarity_matrix(a_side, b[:50])
        eo, eka, ekb = sm.matrix(ids, t, a_side, b[:50])
        assert np.array_equal(gka, eka) and np.array_equal(gkb, ekb), what
        _same_floats(go, eo, what + " matrix")
    qs = np.concatenate([rng.standard_normal((10, d)).astype(np.float32), t[:4] * np.float32(2.0 ** 60)])
    got = vec.assign(qs, b[:100])
    assert asm.same(got, asm.exact_assign(ids, t, qs, b[:100])), what + " exact_assign"
    vec.close()


def _texts(ids, rng):
    out = []
    for L in (1, 2, 3, 5, 7, 64):
        for _ in range(3):
            out.append(rng.choice(ids, L).astype(np.int32))
    out[4][0] = N_C + 9                        # an id without a row
    out.append(np.empty(0, np.int32))
    return out


@pytest.mark.parametrize("exp2", C_EXPS + (-120,))
@pytest.mark.parametrize("d", sorted(IVF_SHAPE))
def test_tokenize_over_small_tables(gpu, oracle, d, exp2):
    """x 2^-64 / 2^-70: the normalisation's sum of squares is subnormal; x 2^-80: it is 0, the length is 0 and the quotients are
    inf / NaN as the reference's are; x 2^-120: the centroid's quotients row / n (n = 3, 7, ...) land in the subnormals."""
    ids, t = _small(d, exp2)
    texts = _texts(ids, np.random.default_rng(200 + d))
    vec = gpu.VectorIndex(ids, t)
    for rule in (tm.TABLE_ORDER, tm.POSITIONAL):
        for normalize in (False, True):
            what = f"d {d} table x 2^{exp2} rule {rule} normalize {normalize}"
            with np.errstate(all="ignore"):
                ev, ec = tm.tokenize(oracle, ids, t, texts, rule, normalize)
            if exp2 == -120 and not normalize:
                assert np.any((ev != 0) & (np.abs(ev) < 2.0 ** -126)), "no subnormal quotient in the centroids"
            if exp2 == -80 and normalize:
                assert np.isinf(ev).any() or np.isnan(ev).any(), "a zero length did not show"
            for unit in ((1, 2) if normalize else (0,)):
                vec.set_option("tokenize_unit", unit)
                gv, gc = vec.tokenize(texts, normalize=normalize, rule=rule)
                assert np.array_equal(gc, ec), what
                _same_floats(gv, ev, f"{what} tokenize_unit {unit}")
            vec.set_option("tokenize_unit", 0)
    vec.close()


@functools.lru_cache(maxsize=None)
def _ivf(d):
    """a small IVF index over the UNIT-scale rows (ids 1 .. N_C): the approximate stage is ordinary, the raw vectors are small"""
    import torch
    from freddy_amd import index_build as ib
    x = torch.from_numpy(ti.scaled_table(0, d=d, n=N_C))
    t = ib.build_ivf_index(x, C=4, m=IVF_SHAPE[d], K=16, train_size=N_C, iters=3, seed=1)
    return t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"]


@pytest.mark.parametrize("exp2", C_EXPS)
@pytest.mark.parametrize("d", sorted(IVF_SHAPE))
def test_post_verification_and_approximate_analogies_over_small_vectors(gpu, oracle, d, exp2):
    import approx_analogy_model as aam
    import pv_model as pm
    ids, t = _small(d, exp2)
    args = _ivf(d)
    ivf, ot, vec = gpu.IVFIndex(*args), oracle.ivf_table(*args), gpu.VectorIndex(ids, t)
    what = f"d {d} vectors x 2^{exp2}"
    qs = ti.scaled_table(0, d=d, n=N_C)[::29][:20].copy()
    k, pvf, W = 5, 4, 2
    exp, _, _ = pm.expected(oracle, pm.ivf_lists(oracle, ot, qs, k * pvf, W), t, ids, qs, k)
    gi, gs = ivf.search_pv(vec, qs, k, pvf, W)
    pm.same(gi, gs, exp, k, what + " search_pv")
    # the analogy's query is vec_normalize(v3 - v1 + v2) of the SMALL vectors: (float)sqrt((double)sq) of a subnormal or zero sq
    triples = np.random.default_rng(300 + d).choice(ids, size=(30, 3)).astype(np.int32)
    with np.errstate(all="ignore"):
        exp, stats, *_ = aam.ivf_expected(oracle, ot, t, ids, triples, 5, 23, W)
    gi, gs = ivf.analogy(vec, triples, 5, 23, W)
    pm.same(gi, gs, exp, 5, what + " ivfadc_analogy")
    assert ivf.last_approx_analogy_stats() == stats, what
    for h in (ivf, vec):
        h.close()
