"""-m gpu: analogy_pair_direction on the device (freddy_gpu_exact_analogy with FREDDY_ANALOGY_PAIR_DIRECTION; analogy.h) against
the numpy model (tests/pair_model.py): ids AND score bits, over the whole table, over "id = ANY(set)" subsets, across the
1024-analogy chunks, at other shapes, and through the host mirror's analogy_pair_direction / analogy()."""
import numpy as np
import pytest

import pair_model as pm
import util

pytestmark = pytest.mark.gpu

N_MAIN = 20_037   # not a multiple of 64


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


def unnormalised(N, d=300, seed=5):
    """util.corpus rows times per-row factors in [0.5, 4]: the original table is not normalised."""
    x = util.corpus(N, d=d).numpy().copy()   # (util.corpus is cached: never write into the shared table)
    f = np.random.default_rng(seed).uniform(0.5, 4.0, size=(N, 1)).astype(np.float32)
    return x * f


@pytest.fixture(scope="module")
def main():
    x = unnormalised(N_MAIN)
    ids = (np.arange(N_MAIN) * 2 + 5).astype(np.int32)
    rng = np.random.default_rng(3)
    t = rng.integers(0, N_MAIN, size=(19, 3))        # 19 analogies: two tiles of 8 and a tile with spare columns
    t[0] = (7, 7, 123)                                # w1 == w2: every score NaN, the lowest ids that are not inputs
    t[1] = (9, 4000, 9)                               # w1 == w3
    t[2] = (300, 301, 5000)
    x[15_001] = x[5000]                               # ... v3 copied under another id: NaN, must come first
    t[3] = (0, 63, 17)                                # inputs in the first block
    t[4] = (N_MAIN - 1, N_MAIN - 5, 20_032)           # inputs in the last block (37 rows)
    triples = ids[t]
    triples[5, 1] = 4                                 # an unknown id (ids are odd)
    x_t = np.ascontiguousarray(x.T)
    ei, es = pm.model(x, ids, triples, 32, x_t=x_t)   # (computed once: the first k of a total order are a prefix of its first 32)
    exp = {k: (ei[:, :k].copy(), es[:, :k].copy()) for k in (1, 5, 32)}
    return dict(x=x, ids=ids, triples=triples, exp=exp)


def test_pair_direction_matches_model(gpu, main):
    x, ids, triples = main["x"], main["ids"], main["triples"]
    idx = gpu.VectorIndex(ids, x)
    for k in (1, 5, 32):
        idx.profile_enable(True)
        got = idx.analogy(triples, k=k, method="pair_direction")
        names = set(idx.profile_read())
        idx.profile_enable(False)
        same(got, main["exp"][k], k)
        assert {"analogy_pair_columns", "analogy_pair_scan", "analogy_merge"} <= names and "analogy_filter" not in names, names
        assert idx.last_analogy_stats() == {"filter_passes": 0, "candidates": 0, "redone_passes": 0}
        live = [q for q in range(len(triples)) if q != 5]
        assert all(not np.isin(got[0][q], triples[q]).any() for q in live), "an input id in a result"
    gi, gs = got
    assert gi[2, 0] == ids[15_001] and np.isnan(gs[2, 0]), "the copy of v3 under another id scores NaN and comes first"
    assert np.isnan(gs[0]).all() and gi[0].tolist() == [i for i in ids[:40].tolist() if i not in triples[0].tolist()][:32]
    assert (gi[5] == -1).all() and np.isneginf(gs[5]).all(), "an unknown id: the SQL's NULL"
    idx.close()


def test_pair_direction_ignores_filter_options(gpu, main):
    x, ids, triples = main["x"], main["ids"], main["triples"]
    idx = gpu.VectorIndex(ids, x)
    c0 = idx.bound_checked()
    for opt, v in (("exact_filter", 0), ("exact_filter", 1), ("check_brackets", 8)):
        idx.set_option(opt, v)
        same(idx.analogy(triples, k=5, method="pair_direction"), main["exp"][5], (opt, v))
        assert idx.last_analogy_stats()["filter_passes"] == 0
    assert idx.bound_checked() == c0 and idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("d,N,k,Q", [(25, 1000, 5, 9), (7, 130, 3, 3), (512, 300, 5, 5), (3029, 6, 8, 9)])
def test_pair_direction_shapes(gpu, d, N, k, Q):
    """Other widths (an odd one, one below the prefetch depth, the widest filtered one, the widest the entry point accepts -- where
    a tile of 8 analogies no longer fits the LDS and 4 are taken), tables of a few blocks, and fewer rows than k + 3 (padding)."""
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, size=(N, 1))).astype(np.float32)
    x[N - 1] = x[2]                                   # a duplicate vector
    if N > 100:
        x[50] = (rng.standard_normal(d) * 1e-21).astype(np.float32)   # differences whose squares are denormal
        x[51] = x[50] * np.float32(1.5)
    ids = (np.arange(N) * 3 + 1).astype(np.int32)
    t = rng.integers(0, N, size=(Q, 3))
    t[0] = (0, 1, 2)
    if N > 100:
        t[1] = (3, 4, 50)
    tr = ids[t]
    idx = gpu.VectorIndex(ids, x)
    got = idx.analogy(tr, k=k, method="pair_direction")
    same(got, pm.model(x, ids, tr, k), (d, N))
    if N < k + 3:
        assert (got[0][0, N - 3:] == -1).all() and np.isneginf(got[1][0, N - 3:]).all()
    idx.close()


def test_pair_direction_d_limit(gpu):
    x = np.random.default_rng(1).standard_normal((8, 3030)).astype(np.float32)
    idx = gpu.VectorIndex(np.arange(1, 9, dtype=np.int32), x)
    with pytest.raises(gpu.FreddyGpuError, match=r"freddy_gpu error -5.*d=3030 too large for the exact analogy"):
        idx.analogy([[1, 2, 3]], k=1, method="pair_direction")
    idx.close()


def test_pair_direction_chunk_loop(gpu):
    """More analogies than one chunk of 1024 holds."""
    N, d, Q = 500, 16, 1030
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((N, d)) * rng.uniform(0.5, 4.0, size=(N, 1))).astype(np.float32)
    ids = (np.arange(N) + 10).astype(np.int32)
    tr = ids[rng.integers(0, N, size=(Q, 3))]
    tr[1027] = (ids[3], ids[3], ids[4])
    tr[500, 0] = 5                                    # unknown: the live analogies are compacted around it
    idx = gpu.VectorIndex(ids, x)
    same(idx.analogy(tr, k=2, method="pair_direction"), pm.model(x, ids, tr, 2), "chunks")
    idx.close()


def test_pair_direction_subsets(gpu, main):
    x, ids = main["x"], main["ids"]
    idx = gpu.VectorIndex(ids, x)
    tr = ids[[[3, 4, 5], [100, 2000, 30]]]
    x_t = np.ascontiguousarray(x.T)
    sub = np.concatenate([ids[50:900], ids[50:60], [4, 10**8], ids[[4]]])   # duplicates, unknown ids, an input inside the set
    for s in (sub, ids[7000:7100]):                   # the second: the inputs lie outside the set
        got = idx.analogy(tr, k=5, method="pair_direction", subset_ids=s)
        same(got, pm.model(x, ids, tr, 5, subset_ids=s, x_t=x_t), len(s))
    got = idx.analogy(tr, k=3, method="pair_direction", subset_ids=np.array([], np.int32))
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    idx.close()


def test_pair_direction_arguments(gpu):
    x = unnormalised(100)
    ids = np.arange(1, 101, dtype=np.int32)
    idx = gpu.VectorIndex(ids, x)
    with pytest.raises(gpu.FreddyGpuError, match="-5"):
        idx.analogy(ids[:3][None], k=33, method="pair_direction")
    with pytest.raises(ValueError):
        idx.analogy(ids[:3][None], k=1, method="pair_directions")
    assert idx.analogy(np.zeros((0, 3), np.int32), k=2, method="pair_direction")[0].shape == (0, 2)
    idx.close()


def test_host_mirror_pair_direction(gpu):
    """google_vecs beside google_vecs_norm (different contents, rows in another order): analogy_pair_direction and analogy() under
    that name answer from the original table, the other methods still from the normalised one."""
    from freddy_amd import udf
    N = 20000
    xn = util.corpus(N).numpy().copy()
    xo = unnormalised(N, seed=9)[::-1].copy()         # other rows under the ids: the two tables differ in more than scale
    ids_all = np.arange(1, N + 1, dtype=np.int32)
    s = udf.Session()
    s.load_vecs_norm(ids_all, xn)
    perm = np.random.default_rng(2).permutation(N - 10)            # google_vecs lacks the ten highest ids, in any row order
    s.load_vecs_original(ids_all[:N - 10][perm], xo[:N - 10][perm])
    vo = gpu.VectorIndex(ids_all[:N - 10], xo[:N - 10])
    vn = gpu.VectorIndex(ids_all, xn)
    for a, b, c in [(11, 222, 3333), (5, 5, 77), (40, 41, 10**7), (19000, 3, 12)]:
        exp = vo.analogy([(a, b, c)], k=1, method="pair_direction")[0][0, 0]
        s.set_analogy_function("analogy_pair_direction")
        assert s.analogy_pair_direction(a, b, c) == s.analogy(a, b, c) == exp
        s.set_analogy_function("analogy_3cosadd")
        assert s.analogy(a, b, c) == s.analogy_3cosadd(a, b, c) == vn.analogy([(a, b, c)], k=1, method="3cosadd")[0][0, 0]
        assert s.analogy_3cosmul(a, b, c) == vn.analogy([(a, b, c)], k=1, method="3cosmul")[0][0, 0]
    assert s.analogy_pair_direction(40, 41, 10**7) == -1
    assert s.analogy_pair_direction(1, 2, N) == -1 and s.analogy_3cosadd(1, 2, N) > 0, "an id only google_vecs_norm has"
    vo.close()
    vn.close()
    s.close()
