"""-m gpu: the exact analogies (freddy_gpu_exact_analogy, analogy.h) against the numpy model (tests/analogy_model.py): ids
AND score bits, on the filter + refine path, the all-exact path and the "id = ANY(set)" path, and through the host mirror's
analogy() / analogy_in() dispatchers."""
import numpy as np
import pytest

import analogy_model as am
import util

pytestmark = pytest.mark.gpu

N_BIG = 200_000


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def same(got, exp, what=""):
    gi, gs = got
    ei, es = exp
    assert np.array_equal(gi, ei), (what, np.nonzero((gi != ei).any(1))[0][:5])
    assert np.array_equal(gs.view(np.uint64), es.view(np.uint64)), (what, np.nonzero((gs.view(np.uint64) != es.view(np.uint64)).any(1))[0][:5])


@pytest.fixture(scope="module")
def big():
    """200 k x 300 (the sample is a strict subset, the filter path runs), 40 analogies (a pass of 32 and one of 8)."""
    x = util.corpus(N_BIG).numpy().copy()   # (util.corpus is cached: never write into the shared table)
    ids = (np.arange(N_BIG) * 2 + 5).astype(np.int32)
    rng = np.random.default_rng(3)
    t = rng.integers(0, N_BIG, size=(40, 3))
    t[:4] = rng.integers(0, 32, size=(4, 3))        # inputs in the first strip, which any sample reads
    t[4] = (7, 7, 123)                               # w1 = w2: v3's own row scores best for 3CosMul (excluded), its copy must win
    x[150_001] = x[123]                              # ... the copy, under another id
    t[5] = (9, 40_000, 9)                            # repeated inputs (w1 = w3)
    return dict(x=x, x_t=np.ascontiguousarray(x.T), ids=ids, rows=t, triples=ids[t])


@pytest.mark.parametrize("method", ["3cosmul", "3cosadd"])
def test_analogy_filter_path_matches_model(gpu, big, method):
    x, ids, triples = big["x"], big["ids"], big["triples"]
    idx = gpu.VectorIndex(ids, x)
    for k in (1, 5, 32):
        got = idx.analogy(triples, k=k, method=method)
        exp = am.model(x, ids, triples, k, method, x_t=big["x_t"])
        same(got, exp, (method, k))
        assert all(not np.isin(got[0][q], triples[q]).any() for q in range(len(triples))), "an input id in a result"
        if k == 5:
            idx.set_option("exact_filter", 0)        # the all-exact kernels: the same lists
            same(idx.analogy(triples, k=k, method=method), got, (method, "all-exact"))
            assert idx.last_analogy_stats()["filter_passes"] == 0
            idx.set_option("exact_filter", 1)
            same(idx.analogy(triples, k=k, method=method), got, (method, "forced filter"))
            idx.set_option("exact_filter", -1)
        st = idx.last_analogy_stats()               # the fast path ran: two passes (32 + 8 analogies), none redone
        assert st["filter_passes"] == 2 and st["redone_passes"] == 0 and st["candidates"] >= k * len(triples), st
    if method == "3cosmul":
        assert got[0][4, 0] == ids[150_001], "the copy of v3 under another id wins; v3's own row is excluded"
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("method", ["3cosmul", "3cosadd"])
def test_analogy_bracket_holds_for_every_row(gpu, big, method):
    """check_brackets bit 3: every row of the table is refined for every analogy, its cosines compared with their brackets."""
    x, ids, triples = big["x"], big["ids"], big["triples"]
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("check_brackets", 8)
    c0 = idx.bound_checked()
    got = idx.analogy(triples, k=5, method=method)
    assert idx.bound_violations() == 0
    assert idx.bound_checked() - c0 == N_BIG * len(triples)
    same(got, am.model(x, ids, triples, 5, method, x_t=big["x_t"]), method)
    idx.close()


@pytest.mark.parametrize("method", ["3cosmul", "3cosadd"])
def test_analogy_small_tables_and_edges(gpu, method):
    N = 3000
    x = util.corpus(N).numpy().copy()
    x[20] = x[21] = x[22] = x[23]                    # equal scores: by ascending id
    ids = (np.arange(N) * 3 + 1).astype(np.int32)
    tr = np.array([[ids[5], ids[5], ids[23]], [ids[1], ids[2], ids[1]], [ids[9], ids[10], 999_999], [ids[100], ids[200], ids[300]]])
    for ef in (-1, 1):                               # all-exact (N < 8192) and the forced filter with a small sample
        idx = gpu.VectorIndex(ids, x)
        idx.set_option("exact_filter", ef)
        for k in (1, 4, 32):
            got = idx.analogy(tr, k=k, method=method)
            same(got, am.model(x, ids, tr, k, method), (ef, k))
            assert (got[0][2] == -1).all() and np.isneginf(got[1][2]).all()   # an unknown id: the SQL's NULL
        idx.close()
    tiny = gpu.VectorIndex(ids[:6], x[:6])           # fewer than k + 3 rows
    got = tiny.analogy(ids[[0, 1, 2]][None], k=8, method=method)
    same(got, am.model(x[:6], ids[:6], ids[[0, 1, 2]][None], 8, method))
    assert (got[0][0, 3:] == -1).all()
    tiny.close()


@pytest.mark.parametrize("d", [416, 512])
def test_analogy_wide_tables(gpu, d):
    """The widest tables exact kNN filters (d <= 512): 3CosMul's three tiles of query fragments fit a CU's LDS up to d = 416;
    beyond, 3CosMul is answered by the all-exact kernels (3CosAdd, one tile, still filters)."""
    N = 9000
    x = util.corpus(N, d=d).numpy().copy()
    ids = (np.arange(N) * 7 + 3).astype(np.int32)
    tr = ids[np.random.default_rng(d).integers(0, N, size=(33, 3))]
    idx = gpu.VectorIndex(ids, x)
    for method in ("3cosmul", "3cosadd"):
        got = idx.analogy(tr, k=5, method=method)
        same(got, am.model(x, ids, tr, 5, method), (d, method))
        st = idx.last_analogy_stats()
        assert st["filter_passes"] == (0 if (method == "3cosmul" and d > 416) else 2) and st["redone_passes"] == 0, (d, method, st)
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("method", ["3cosmul", "3cosadd"])
def test_analogy_nan_scores_sort_first(gpu, method):
    """A row holding a NaN scores NaN: it sorts first (PostgreSQL's float8 order), equal NaNs by id (a non-finite table: the
    all-exact kernels)."""
    N = 9000
    x = util.corpus(N).numpy().copy()
    x[4321, 17] = np.nan
    x[77, 3] = np.nan
    ids = (np.arange(N) + 1).astype(np.int32)
    tr = ids[[[1, 2, 3], [10, 20, 30]]]
    idx = gpu.VectorIndex(ids, x)
    got = idx.analogy(tr, k=4, method=method)
    same(got, am.model(x, ids, tr, 4, method), method)
    assert got[0][:, :2].tolist() == [[ids[77], ids[4321]]] * 2 and np.isnan(got[1][:, :2]).all()
    idx.close()


def test_analogy_in_subsets(gpu):
    N = 20000
    x = util.corpus(N).numpy().copy()
    ids = (np.arange(N) + 10).astype(np.int32)
    idx = gpu.VectorIndex(ids, x)
    tr = ids[[[3, 4, 5], [100, 2000, 30]]]
    sub = np.concatenate([ids[50:900], ids[50:60], [5, 10**8], ids[[4]]])   # duplicates, unknown ids, an input inside the set
    for method in ("3cosmul", "3cosadd"):
        for s in (sub, ids[7000:7100]):              # the second: the inputs lie outside the set
            got = idx.analogy(tr, k=5, method=method, subset_ids=s)
            same(got, am.model(x, ids, tr, 5, method, subset_ids=s), method)
        got = idx.analogy(tr, k=3, method=method, subset_ids=np.array([], np.int32))
        assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    idx.close()


def test_analogy_arguments(gpu):
    x = util.corpus(100).numpy().copy()
    ids = np.arange(1, 101, dtype=np.int32)
    idx = gpu.VectorIndex(ids, x)
    with pytest.raises(gpu.FreddyGpuError, match="-5"):
        idx.analogy(ids[:3][None], k=33)
    with pytest.raises(ValueError):
        idx.analogy(ids[:3][None], k=1, method="3cosfoo")
    assert idx.analogy(np.zeros((0, 3), np.int32), k=2)[0].shape == (0, 2)
    idx.close()


def test_host_mirror_dispatch(gpu, oracle):
    from freddy_amd import udf
    N = 20000
    x = util.corpus(N).numpy().copy()
    ids_all = np.arange(1, N + 1, dtype=np.int32)
    s = udf.Session()
    s.load_vecs_norm(ids_all, x)
    pq = util.pq_tables(N=N, K=256)
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    vi = gpu.VectorIndex(ids_all, x)
    trip = [(11, 222, 3333), (5, 5, 77), (40, 41, 10**7)]
    subset = ids_all[1000:3000]
    assert s.get_analogy_function_name() == "analogy_3cosadd" and s.get_analogy_in_function_name() == "analogy_3cosadd_in"
    for a, b, c in trip:
        exp_add = vi.analogy([(a, b, c)], k=1, method="3cosadd")[0][0, 0]
        exp_mul = vi.analogy([(a, b, c)], k=1, method="3cosmul")[0][0, 0]
        exp_in = vi.analogy([(a, b, c)], k=1, method="3cosadd", subset_ids=subset)[0][0, 0]
        s.set_analogy_function("analogy_3cosadd")
        s.set_analogy_in_function("analogy_3cosadd_in")
        assert s.analogy(a, b, c) == s.analogy_3cosadd(a, b, c) == exp_add
        assert s.analogy_in(a, b, c, subset) == s.analogy_3cosadd_in(a, b, c, subset) == exp_in
        s.set_analogy_function("analogy_3cosmul")
        assert s.analogy(a, b, c) == s.analogy_3cosmul(a, b, c) == exp_mul
        s.set_analogy_function("analogy_3cosadd_pq")
        assert s.analogy(a, b, c) == s.analogy_3cosadd_pq(a, b, c)
        s.set_analogy_in_function("analogy_3cosadd_in_pq")
        assert s.analogy_in(a, b, c, subset) == s.analogy_3cosadd_in_pq(a, b, c, subset)
    assert s.analogy_3cosadd(1, 2, 10**7) == -1 and s.analogy_3cosmul(10**7, 2, 3) == -1
    s.set_analogy_function("no_such_analogy")
    with pytest.raises(udf.FreddyError, match=r"function no_such_analogy\(unknown, unknown, unknown\) does not exist"):
        s.analogy(1, 2, 3)
    s.set_analogy_in_function("analogy_3cosadd")   # a three-argument function: analogy_in finds no such function
    with pytest.raises(udf.FreddyError, match=r"function analogy_3cosadd\(unknown, unknown, unknown, character varying\[\]\) does not exist"):
        s.analogy_in(1, 2, 3, subset)
    vi.close()
    s.close()
