"""The oracle's answers for non-finite inputs (NaN, -NaN, +-Inf in queries, codebooks, centroids and rows), pinned against
independent Python models written from the rules (plain `<` comparisons in binary32: a NaN is never smaller and nothing is
smaller than a NaN).  These answers are the reference of tests/test_gpu_nonfinite.py.  The same cases run once more against
the ASan + UBSan build of the oracle (as tests/test_sanitizers.py drives it), so an input for which the oracle reads out of
bounds or does not end shows up here and not on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import util
from test_oracle import as_list, py_insert, py_stream

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, C = 400, 16, 4
SHAPES = [(12, 3), (25, 5)]     # (d, m)


# ---------------------------------------------------------------------------------------------
# models (from the rule; vectorised over rows, every step rounded to binary32 as index_utils.c:500-508 does)
# ---------------------------------------------------------------------------------------------
def np_sqdist(a, B):
    """squareDistance of a against every row of B: t = a - b, p = t * t, acc = acc + p, one rounding each."""
    a, B = np.asarray(a, f32), np.asarray(B, f32)
    acc = np.zeros(B.shape[0], f32)
    with np.errstate(all="ignore"):
        for j in range(a.size):
            t = a[j] - B[:, j]
            acc = acc + t * t
    return acc


def py_lut(q, cb):
    m, K_, s = cb.shape
    return np.stack([np_sqdist(q[p * s:(p + 1) * s], cb[p]) for p in range(m)])     # [m][K]


def py_adc(lut, codes):
    acc = np.zeros(codes.shape[0], f32)
    with np.errstate(all="ignore"):
        for l in range(codes.shape[1]):
            acc = acc + lut[l][codes[:, l]]
    return acc


def py_argmin_strict(dists, start=None):
    """The reference's argmin: from `start` (None: the first value, whatever it is) by strict <, lowest index on ties."""
    best, bd = -1, start
    for j, d in enumerate(dists):
        if (best < 0 and start is None) or d < bd:
            best, bd = j, d
    return best


def py_pq_search(t, q, k, sentinel, rows=None):
    lut = py_lut(q, t["codebook"])
    rows = np.arange(t["ids"].size) if rows is None else rows
    return py_stream(py_adc(lut, t["codes"][rows]), t["ids"][rows], k, sentinel)


def py_ivfadc_search(t, q, k, W, sentinel, rule):
    """freddy.c:174-393 with the oracle's two commented departures (unused slots of the cell list are skipped; no cell left ends it)."""
    coarse, lo = t["coarse"], t["list_off"]
    black = np.zeros(coarse.shape[0], bool)
    tk, maxd, found = [(-1, f32(sentinel))] * k, f32(sentinel), 0
    while found < k:
        sel, mind = [(-1, f32(100.0))] * W, f32(1000.0)
        for j, dist in enumerate(np_sqdist(q, coarse)):
            if not black[j] and dist < mind:
                py_insert(sel, dist, j)
                mind = sel[W - 1][1]
        cells = [c for c, _ in sel if c >= 0]
        if not cells:
            break
        black[cells] = True
        with np.errstate(all="ignore"):
            luts = {c: py_lut((q - coarse[c]).astype(f32), t["codebook"]) for c in cells}
        cand = []
        for c in cells:
            r = np.arange(lo[c], lo[c + 1])
            cand += list(zip(t["ids"][r].tolist(), py_adc(luts[c], t["codes"][r])))
        cand.sort(key=lambda e: e[0])
        accepted = 0
        for i, dist in cand:
            if dist < maxd:
                py_insert(tk, dist, i)
                maxd = tk[k - 1][1]
                accepted += 1
        found += accepted if rule else len(cand)
    return tk


def py_ivfadc_batch_search(t, q, k):
    """freddy.c:679-999 for one query (queries do not interact): the nearest unused cell by strict < from 1000, sentinel 100,
    found = accepted rows; a query with no cell left is retired."""
    coarse, lo = t["coarse"], t["list_off"]
    black = np.zeros(coarse.shape[0], bool)
    tk, maxd, found = [(-1, f32(100.0))] * k, f32(100.0), 0
    while found < k:
        dist = np_sqdist(q, coarse)
        pick = py_argmin_strict([f32(np.inf) if black[j] else dist[j] for j in range(len(dist))], start=f32(1000.0))
        if pick < 0 or black[pick]:
            break
        black[pick] = True
        with np.errstate(all="ignore"):
            lut = py_lut((q - coarse[pick]).astype(f32), t["codebook"])
        r = np.arange(lo[pick], lo[pick + 1])
        for i, dd in zip(t["ids"][r].tolist(), py_adc(lut, t["codes"][r])):
            if dd < maxd:
                py_insert(tk, dd, i)
                maxd = tk[k - 1][1]
                found += 1
    return tk


def py_exact_knn(x, ids, q, k):
    """ORDER BY similarity DESC, id ASC in PostgreSQL's float4 order: NaN = NaN, and NaN above every number, +Inf included.
    A sort, not the oracle's insertion: (is a number, -similarity, id) ascending."""
    sims = []
    for r in range(x.shape[0]):
        sim = f32(0)
        with np.errstate(all="ignore"):
            for a, b in zip(q, x[r]):
                sim = f32(sim + f32(a * b))
        sims.append(sim)
    order = sorted(range(len(sims)), key=lambda r: (0, 0.0, int(ids[r])) if np.isnan(sims[r]) else (1, -float(sims[r]), int(ids[r])))
    return [(int(ids[r]), sims[r]) for r in order[:k]]


# ---------------------------------------------------------------------------------------------
# tables and poisons
# ---------------------------------------------------------------------------------------------
def _tables(d, m, seed=0):
    rng = np.random.default_rng(100 * d + seed)
    s = d // m
    x = (rng.standard_normal((N, d)) * 0.3).astype(f32)
    coarse = x[rng.choice(N, C, replace=False)].copy()
    cell = np.array([py_argmin_strict(np_sqdist(v, coarse)) for v in x])
    order = np.argsort(cell, kind="stable")
    cb = (rng.standard_normal((m, K, s)) * 0.3).astype(f32)
    codes = rng.integers(0, K - 1, (N, m)).astype(np.int16)      # code K - 1 is used by no row
    codes[:120, 0] = 2                                           # (position 0, code 2): used by at least 100 rows
    list_off = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=C))]).astype(np.int32)
    ids = np.arange(1, N + 1, dtype=np.int32)
    return dict(x=x, coarse=coarse, codebook=cb, ids=ids, codes=codes[order], list_off=list_off, pq_codes=codes)


def _queries(t, d, m, seed=3):
    rng = np.random.default_rng(seed)
    base = t["x"][rng.choice(N, 2 * len(util.QUERY_POISONS) + 2, replace=False)]
    out = [base[-1], base[-2]]
    for j, kind in enumerate(util.QUERY_POISONS):
        out.append(util.poison_query(base[2 * j], kind, m, rng, "first"))
        out.append(util.poison_query(base[2 * j + 1], kind, m, rng, "last"))
    return np.stack(out)


TABLE_POISONS = ("healthy", "centroid_nan", "centroid_inf", "codeword_nan_used", "codeword_nan_unused", "codeword_inf", "slice_nan")


def _poison_table(t, kind):
    t = {k_: v.copy() for k_, v in t.items()}
    if kind == "centroid_nan":
        t["coarse"][int(np.argmax(np.diff(t["list_off"]))), 1] = np.nan
    elif kind == "centroid_inf":
        t["coarse"][int(np.argmax(np.diff(t["list_off"]))), -1] = np.inf
    elif kind == "codeword_nan_used":
        t["codebook"][0, 2, 0] = np.nan
    elif kind == "codeword_nan_unused":
        t["codebook"][0, K - 1, 0] = np.nan
    elif kind == "codeword_inf":
        t["codebook"][0, 2, 1] = np.inf
    elif kind == "slice_nan":
        t["codebook"][-1] = np.nan
    return t


def _same(got, exp, what):
    got = as_list(got)
    assert [i for i, _ in got] == [i for i, _ in exp], what
    # (a NaN entry -- exact_knn only -- is compared as "a NaN": an invalid operation gives 0xffc00000 on x86 and 0x7fc00000 elsewhere)
    bits = lambda l: [0x7fc00000 if np.isnan(x) else int(f32(x).view(np.uint32)) for _, x in l]
    assert bits(got) == bits(exp), what


# ---------------------------------------------------------------------------------------------
# the searches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", SHAPES)
@pytest.mark.parametrize("poison", TABLE_POISONS)
def test_pq_search_nonfinite(oracle, d, m, poison):
    """pq_search and pq_search_in_batch: a NaN anywhere in a row's sum makes the row's distance NaN, which is never below the
    running maximum -- the row is skipped; an all-NaN table gives the all-(-1, sentinel) list."""
    t = _poison_table(_tables(d, m), poison)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["pq_codes"])
    qs = _queries(t, d, m)
    tt = dict(t, codes=t["pq_codes"])
    sub = np.concatenate([t["ids"][::3], t["ids"][:5], [N + 7]]).astype(np.int32)
    rows = np.unique(sub[sub <= N]) - 1
    for tl in (True, False):
        batch = oracle.pq_search_in_batch(ot, qs, 5, sub, use_target_lists=tl)
        for qi, q in enumerate(qs):
            _same(batch[qi], py_pq_search(tt, q, 5, 1000.0, rows), f"pq_search_in_batch {poison} tl={tl} query {qi}")
    for qi, q in enumerate(qs):
        _same(oracle.pq_search(ot, q, 5), py_pq_search(tt, q, 5, 100.0), f"pq_search {poison} query {qi}")
    if poison == "slice_nan":
        assert (oracle.pq_search(ot, qs[0], 5)["id"] == -1).all()
    if poison == "codeword_nan_used":
        assert not set(oracle.pq_search(ot, qs[0], N)["id"].tolist()) & set(t["ids"][:120].tolist())


@pytest.mark.parametrize("d,m", SHAPES)
@pytest.mark.parametrize("poison", TABLE_POISONS)
def test_ivfadc_search_nonfinite(oracle, d, m, poison):
    """ivfadc_search under both found rules and ivfadc_batch_search: a query or centroid whose coarse distance is NaN or +Inf
    selects no such cell (NaN < 1000 and Inf < 1000 are false); a query with no selectable cell gets the all-(-1, sentinel)
    list; found rule 1 over rows that are all NaN keeps probing until no cell is left."""
    t = _poison_table(_tables(d, m), poison)
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    qs = _queries(t, d, m)
    for k, W, rule, sent in ((5, 2, 0, 1000.0), (5, 1, 1, 100.0), (7, 3, 1, 1000.0)):
        got = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
        for qi, q in enumerate(qs):
            _same(got[qi], py_ivfadc_search(t, q, k, W, sent, rule), f"ivfadc {poison} k={k} W={W} rule={rule} query {qi}")
    got = oracle.ivfadc_batch_search(ot, qs, 5)
    for qi, q in enumerate(qs):
        _same(got[qi], py_ivfadc_batch_search(t, q, 5), f"ivfadc_batch_search {poison} query {qi}")
    if poison == "healthy":
        for qi in range(2, len(qs)):     # every poisoned query: no cell, the empty list
            assert (got[qi]["id"] == -1).all() and (got[qi]["dist"] == f32(100.0)).all(), qi


@pytest.mark.parametrize("d,m", SHAPES)
def test_encode_grouping_kmeans_nonfinite(oracle, d, m):
    """The argmins: encode / assign_coarse start from the FIRST entry whatever its distance and move on strict <: an all-NaN
    sub-vector takes code 0, and a NaN codeword at code 0 is never left (nothing is < NaN).  grouping_pq starts from 100: a
    row whose every distance is NaN gets group -1.  kmeans: a NaN training row joins cluster 0 and turns its centroid NaN."""
    t = _tables(d, m)
    s = d // m
    vecs = np.concatenate([_queries(t, d, m), t["x"][:40]])
    for poison in ("healthy", "codeword_nan_used", "codeword_inf", "slice_nan", "code0_nan"):
        tp = _poison_table(t, poison)
        if poison == "code0_nan":
            tp["codebook"][1, 0, 0] = np.nan
        got = oracle.encode_pq(tp["codebook"], vecs)
        exp = np.array([[py_argmin_strict(np_sqdist(v[p * s:(p + 1) * s], tp["codebook"][p])) for p in range(m)] for v in vecs])
        assert np.array_equal(got, exp), poison
        if poison == "code0_nan":
            assert (got[:, 1] == 0).all()
        ot = oracle.pq_table(tp["codebook"], tp["ids"], tp["pq_codes"])
        gi, gg = oracle.grouping_pq(ot, vecs[:9], tp["ids"])
        for r in range(N):
            dist = [py_adc(py_lut(g, tp["codebook"]), tp["pq_codes"][r:r + 1])[0] for g in vecs[:9]] if r < 130 or r % 9 == 0 else None
            if dist is not None:
                assert gg[r] == py_argmin_strict(dist, start=f32(100.0)), (poison, r)
        if poison == "slice_nan":
            assert (gg == -1).all()
    for cpoison in ("healthy", "centroid_nan", "centroid_inf"):
        tp = _poison_table(t, cpoison)
        got = oracle.assign_coarse(tp["coarse"], vecs)
        assert got.tolist() == [py_argmin_strict(np_sqdist(v, tp["coarse"])) for v in vecs], cpoison
    coarse0 = t["coarse"].copy(); coarse0[0, 0] = np.nan
    assert (oracle.assign_coarse(coarse0, vecs) == 0).all()
    # k-means: model = assign by the argmin above, mean = sequential binary32 sum / count, empty clusters keep their centroid
    train = np.concatenate([t["x"][:60], _queries(t, d, m)[[2, 6]]])     # a NaN row and a +Inf row among the training rows
    init = np.array([3, 17, 31, 45], np.int32)
    gc, ga = oracle.kmeans(train, 4, 3, init)
    cent = train[init].copy()
    for it in range(4):
        a = np.array([py_argmin_strict(np_sqdist(v, cent)) for v in train])
        if it == 3:
            break
        for c in range(4):
            rows = np.nonzero(a == c)[0]
            if rows.size:
                acc = np.zeros(d, f32)
                with np.errstate(all="ignore"):
                    for r in rows:
                        acc = acc + train[r]
                    cent[c] = acc / f32(rows.size)
    assert np.array_equal(ga, a)
    assert np.array_equal(gc.view(np.uint32) & 0x7fffffff, cent.view(np.uint32) & 0x7fffffff)   # (a NaN's sign is not pinned)
    assert np.isnan(gc[0]).any() and ga[-2] == 0


@pytest.mark.parametrize("d", [12, 25])
def test_exact_knn_nonfinite(oracle, d):
    """exact_knn: NaN similarities (a NaN, or opposite infinities, in the row or the query) sort first as PostgreSQL's ORDER BY
    ... DESC puts them, by ascending id; +Inf / -Inf similarities sort as numbers."""
    rng = np.random.default_rng(d)
    x = rng.standard_normal((200, d)).astype(f32)
    ids = (np.arange(200) * 2 + 3).astype(np.int32)
    x[20, 3] = np.nan
    x[90, d - 1] = np.inf
    x[150] *= f32(3e19)        # the row's norm overflows; products with ordinary queries stay finite
    x[151] = f32(3e38)         # products that overflow to +-Inf and then cancel to NaN
    prng = np.random.default_rng(2)
    qs = np.stack([x[5], x[150]] + [util.poison_query(x[30 + j], kind, 1, prng) for j, kind in enumerate(util.QUERY_POISONS)])
    for k in (1, 5, 30, 200):
        for qi, q in enumerate(qs):
            got = oracle.exact_knn(x, ids, q, k)
            exp = py_exact_knn(x, ids, q, k)
            _same(got, exp, f"exact_knn d={d} k={k} query {qi}")
    got = oracle.exact_knn(x, ids, x[5], 30)     # a healthy query: the NaN row leads its list
    n_nan = int(np.isnan(got["dist"]).sum())     # (row 151's products overflow and may cancel to a second NaN)
    assert got["id"][0] == ids[20] and n_nan >= 1 and np.isnan(got["dist"][:n_nan]).all() and (np.diff(got["id"][:n_nan]) > 0).all()


# ---------------------------------------------------------------------------------------------
# the approximate kNN-join: which non-finite inputs the oracle is defined for
# ---------------------------------------------------------------------------------------------
def join_tables(seed=7):
    from freddy_amd import index_build as ib
    x = util.shape_corpus(500, 12)
    return ib.build_ivpq_index(x, m=3, K=16, k_coarse=4, train_size=500, iters=3, seed=seed), x.numpy()


def test_knn_join_nonfinite_is_defined_and_independent(oracle):
    """ivpq_search_in with poisoned queries ends, and (the heap's order under NaN keys aside) answers every healthy query as
    in a batch without the poisoned ones: a healthy query is retired in round one of either call, and only the queries still
    active (the poisoned ones, which accept no row) go through further rounds.  Under the sanitizer build this
    is also the check that the literal heap (index_utils.c:118-155) stays inside its array when its keys do not order."""
    t, x = join_tables()
    ot = oracle.ivpq_table(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])
    healthy = x[::37][:14].astype(f32)
    qs = healthy.copy()
    rng = np.random.default_rng(1)
    bad = [1, 3, 4, 7, 9, 12]
    for j, r in enumerate(bad):
        qs[r] = util.poison_query(qs[r], util.QUERY_POISONS[j], 3, rng, "first" if j % 2 else "last")
    good = [r for r in range(14) if r not in bad]
    targets = t["ids"][::2]
    for method in (0, 1, 2):
        for tl in (True, False):
            got, it = oracle.ivpq_search_in(ot, qs, 3, targets, 2, 4, method, use_target_lists=tl, confidence=0.8)
            ref, it0 = oracle.ivpq_search_in(ot, healthy, 3, targets, 2, 4, method, use_target_lists=tl, confidence=0.8)
            assert it0 == 1, "the independence argument needs single-round calls"
            assert np.array_equal(got[good].view(np.uint8), ref[good].view(np.uint8)), (method, tl, it)
            for r in bad:     # NaN and Inf distances are never accepted: whatever cells were taken, no row enters
                assert (got[r]["id"] == -1).all() and (got[r]["dist"] == f32(1000.0)).all(), (method, tl, r)


# ---------------------------------------------------------------------------------------------
# the same cases under ASan + UBSan
# ---------------------------------------------------------------------------------------------
def test_nonfinite_cases_under_asan_and_ubsan():
    from test_sanitizers import _run_under_asan
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan"])
    so = os.path.join(ROOT, "oracle", "_asan", "libfreddy_oracle_asan.so")
    cp = _run_under_asan(["tests/test_nonfinite_cpu.py", "-k", "not under_asan"], {"FREDDY_ORACLE_SO": so})
    assert " passed" in cp.stdout
