"""-m gpu: every entry point at table shapes other than 300-d / m = 12 (the library is shape-generic: the C ABI takes any
d, m, K with d % m == 0, the reference ships a 25-d / m = 5 index and an m = 30 / K = 32 one).  Each case compares with the
CPU oracle given the same arrays -- ids, ranks and distance / similarity bits -- and, where the dispatch depends on the shape,
reads the handle's profile to name the kernel that ran: a case that silently takes the kernel of the 300-d tests fails."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

E_LIMIT = "freddy_gpu error -5"   # include/freddy_gpu.h FREDDY_E_LIMIT as gpu._check words it


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _profiled(idx, call):
    """(result of call(), names of the kernels it launched)"""
    idx.profile_enable(True)
    out = call()
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return out, names


# ---------------------------------------------------------------------------------------
# 1. exact kNN over d
# ---------------------------------------------------------------------------------------
def _exact_table(d, N, scale=1.0):
    x = (util.shape_corpus(N, d).numpy() * np.float32(scale)).astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]              # duplicate rows beside those of the corpus: equal similarities, ties by id
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::N // 70][:70].copy()                   # 70 queries: a full filter pass of 64 and one of 6; tiles of 16 and 8
    qs[3] = -qs[3]                                  # negative similarities
    qs[6] = x[100]                                  # a query with exact copies in the table
    return x, ids, qs


def _exact_expect(oracle, x, ids, qs, kmax, sub=None):
    """The oracle's lists of kmax entries: ORDER BY similarity DESC, id ASC is a total order, so the list for k is their prefix."""
    return [oracle.exact_knn(x, ids, q, kmax, sub) for q in qs]


_exact_same = util.assert_exact_lists   # (shared with tests/test_gpu_selection_widths.py)


@pytest.mark.parametrize("d", [16, 64, 100, 304, 512])
def test_exact_knn_filter_eligible_d(gpu, oracle, d):
    """d % 4 == 0, 16 <= d <= 512: the filter + refine path (exact2.h) engages unforced from 8192 rows on.  d = 16: one
    fragment tile; 64, 304, 512: whole tiles, no padded dimension; 100: T = 7 with twelve padded dimensions; 304 and 512 take
    exf_eps_factor's 6e-5.  Unforced, forced and switched off give the same lists, the oracle's; the profile says which ran."""
    N = 8192 + 40
    x, ids, qs = _exact_table(d, N)
    exp = _exact_expect(oracle, x, ids, qs, 32)
    idx = gpu.VectorIndex(ids, x)
    for Q in (1, 8, 9, 70):
        for k in (1, 5, 32):
            for mode in (-1, 1, 0):
                idx.set_option("exact_filter", mode)
                (gi, gs), names = _profiled(idx, lambda: idx.search(qs[:Q], k))
                _exact_same(gi, gs, exp, k, f"d={d} Q={Q} k={k} exact_filter={mode}")
                if mode == 0:
                    assert "exact_filter" not in names and "exact_scan" in names, (d, Q, k, mode, sorted(names))
                else:
                    assert "exact_filter" in names and "exact_refine" in names, (d, Q, k, mode, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("d,scale", [(16, 1.0), (64, 1.0), (512, 1.0), (512, 3000.0), (512, 2e-4)])
def test_exact_knn_bracket_holds_for_every_row_over_d(gpu, oracle, d, scale):
    """check_brackets = 4: every (query, row) pair goes through the refine stage, which compares the MFMA value with the
    reference's similarity.  d = 16 (one tile), 64 (no padding), 512 (the 6e-5 factor; also unnormalised tables, whose elements
    exercise the power-of-two operand scale)."""
    N = 8192 + 77
    x, ids, qs = _exact_table(d, N, scale)
    x[1000:1040] *= np.float32(37.5)                # a few long rows: the norm bound is their norm
    x[2000:2020] = 0.0
    rng = np.random.default_rng(d)
    qs = np.concatenate([qs[:10], (rng.standard_normal((2, d)) * 0.01 * scale).astype(np.float32)])
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("check_brackets", 4)
    (gi, gs), names = _profiled(idx, lambda: idx.search(qs, 5))
    assert "exact_filter" in names, sorted(names)
    assert idx.bound_violations() == 0
    assert idx.bound_checked() == qs.shape[0] * N
    _exact_same(gi, gs, _exact_expect(oracle, x, ids, qs, 5), 5, f"every row d={d} scale={scale}")
    idx.close()


def test_exact_knn_bracket_at_the_worst_rounding_of_the_chain(gpu, oracle):
    """The widest gap between the reference's chain and the true product that a 512-d input can open: x = q = (1, t, ..., t)
    with t * t just below (above) half an ulp of 1 -- every one of the 511 additions rounds the same way, the chain returns 1
    (1 + 511 * 2^-23) while the product is 1 + 511 t^2: 3.0e-5 |x||q| apart, half of the bracket's 6e-5 and the term the
    factor grows with d for.  No other row is longer, so eps is not slack.  Every row refined: no violation, the oracle's lists."""
    d, N = 512, 8192 + 13
    x, ids, qs = _exact_table(d, N)
    lo, hi = np.float32(np.sqrt(0.98 * 2.0 ** -24)), np.float32(np.sqrt(1.02 * 2.0 ** -24))
    down = np.full(d, lo, np.float32); down[0] = 1.0
    up = np.full(d, hi, np.float32); up[0] = 1.0
    assert oracle.cosine_similarity_bytea(down, down) == np.float32(1.0)
    assert oracle.cosine_similarity_bytea(up, up) == np.float32(1.0 + 511 * 2.0 ** -23)
    for v in (down, up):
        gap = abs(float(oracle.cosine_similarity_bytea(v, v)) - float(np.dot(v.astype(np.float64), v.astype(np.float64))))
        assert gap > 2.9e-5 * float(np.dot(v.astype(np.float64), v.astype(np.float64))), gap
    x[4000], x[4001], x[4002], x[4003] = down, up, -down, -up
    qs = np.stack([down, up, -down, -up, qs[0], qs[3]])
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("check_brackets", 4)
    (gi, gs), names = _profiled(idx, lambda: idx.search(qs, 5))
    assert "exact_filter" in names, sorted(names)
    assert idx.bound_violations() == 0
    assert idx.bound_checked() == qs.shape[0] * N
    _exact_same(gi, gs, _exact_expect(oracle, x, ids, qs, 5), 5, "worst rounding of the chain")
    assert gi[0, 0] in (ids[4000], ids[4001]) and gi[2, 0] in (ids[4002], ids[4003])
    idx.close()


@pytest.mark.parametrize("d", [4, 12, 25, 301, 516, 768, 1024])
def test_exact_knn_other_d_takes_the_all_exact_scan(gpu, oracle, d):
    """d below 16, not a multiple of 4, or above 512: no filter (forced or not), exact_scan_kernel is the only path.  Tiles of 8
    queries (Q <= 8, and k = 1025: V = 16) and of 16 (Q = 9, 70); V = 1, 2, 4 and 16 (k = 1, 5, 33, 200, 1025); the second
    FLOOR pass (k = 1025).  From d = 513 on the tile of 16 queries asks for more than 64 KiB of dynamic LDS."""
    N = 8192
    x, ids, qs = _exact_table(d, N)
    exp = _exact_expect(oracle, x, ids, qs, 1025)
    idx = gpu.VectorIndex(ids, x)
    for mode in (-1, 1):
        idx.set_option("exact_filter", mode)
        for Q in (1, 8, 9, 70):
            for k in (1, 5, 33, 200, 1025) if mode == -1 else (5,):
                (gi, gs), names = _profiled(idx, lambda: idx.search(qs[:Q], k))
                assert "exact_filter" not in names and "exact_scan" in names and "exact_merge" in names, (d, Q, k, sorted(names))
                _exact_same(gi, gs, exp, k, f"d={d} Q={Q} k={k} exact_filter={mode}")
    idx.close()


@pytest.mark.parametrize("d", [64, 768])
def test_exact_knn_subsets_over_d(gpu, oracle, d):
    """id = ANY(set) with duplicates and unknown ids at a filter-eligible d and at one that is not (subsets always take the
    all-exact scan over the gathered rows); a set of fewer rows than k pads with (-1, -inf)."""
    N = 8192
    x, ids, qs = _exact_table(d, N)
    idx = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(2)
    sub = np.concatenate([ids[rng.choice(N, 700, replace=False)], ids[:30], ids[:30], np.array([4, 10**8, -7], np.int32)])
    for Q, k in ((9, 10), (3, 200), (70, 1)):
        (gi, gs), names = _profiled(idx, lambda: idx.search(qs[:Q], k, subset_ids=sub))
        assert "exact_scan" in names and "exact_filter" not in names, sorted(names)
        _exact_same(gi, gs, _exact_expect(oracle, x, ids, qs[:Q], k, sub), k, f"subset d={d} Q={Q} k={k}")
    few = np.array([ids[5], ids[5], ids[77], 10**8, ids[4000]], np.int32)
    gi, gs = idx.search(qs[:9], 8, subset_ids=few)
    assert (gi[:, 3:] == -1).all() and np.isneginf(gs[:, 3:]).all()
    _exact_same(gi, gs, _exact_expect(oracle, x, ids, qs[:9], 8, few), 8, f"three rows, k = 8, d={d}")
    idx.close()


def test_exact_knn_append_rows_d64(gpu, oracle):
    """append_rows at d = 64 (four tiles, no padding): the first append starts inside a 32-row strip of the fragment-order copy
    and ends inside another; the second brings a larger element, which changes the scale and lays the whole copy out again."""
    d, N0, N1, N2 = 64, 8192 + 8, 8192 + 8 + 45, 8192 + 8 + 45 + 100
    x, ids, qs = _exact_table(d, N2)
    assert N0 % 32 and N1 % 32 and N0 // 32 != N1 // 32
    x[N1 + 5] *= np.float32(300.0)
    idx = gpu.VectorIndex(ids[:N0], x[:N0])
    qs = np.concatenate([qs[:9], x[N0 + 3:N0 + 5], x[N1 + 5:N1 + 6]])
    for lo, n in ((N0, N1), (N1, N2)):
        idx.append_rows(ids[lo:n], vectors=x[lo:n])
        (gi, gs), names = _profiled(idx, lambda: idx.search(qs, 5))
        assert "exact_filter" in names, sorted(names)
        _exact_same(gi, gs, _exact_expect(oracle, x[:n], ids[:n], qs, 5), 5, f"after the append to {n} rows")
    assert idx.bound_violations() == 0
    idx.close()


def test_exact_knn_widest_tables(gpu, oracle):
    """exact_scan_kernel's dynamic LDS is d * QT * 4 bytes of queries + 4 * QT * 64 * 8 of staging, and a CU has 160 KiB: tiles
    of QT = 16 queries fit up to d = 2048, tiles of 8 up to d = 4608.  Batches of more than 8 queries over 2048 < d <= 4608 take
    tiles of 8; freddy_gpu_pin_vectors refuses d > 4608 with FREDDY_E_LIMIT and a message that names d.  The last accepted and
    the first other value on each side: lists equal the oracle's, or the refusal -- never a HIP launch error."""
    rng = np.random.default_rng(11)
    N = 300
    ids = np.arange(1, N + 1, dtype=np.int32)
    for d in (2048, 2052, 4608):
        x = rng.standard_normal((N, d)).astype(np.float32)
        x[200] = x[7]
        idx = gpu.VectorIndex(ids, x)
        qs = x[:11].copy()
        for Q, k in ((8, 5), (9, 5), (11, 200), (9, 1025)):
            (gi, gs), names = _profiled(idx, lambda: idx.search(qs[:Q], k))
            assert "exact_scan" in names and "exact_filter" not in names, (d, sorted(names))
            _exact_same(gi, gs, _exact_expect(oracle, x, ids, qs[:Q], k), k, f"d={d} Q={Q} k={k}")
        idx.close()
    with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*d=4609"):
        gpu.VectorIndex(ids[:4], np.zeros((4, 4609), np.float32))


def test_analogy_widest_tables(gpu):
    """freddy_gpu_exact_analogy refuses a table whose all-exact scan would not fit the LDS for either method
    (an_scan_kernel<3, 4>: 48 d + 18432 bytes within 160 KiB, d <= 3029): d = 3029 answers like the model, d = 3030 is refused
    with FREDDY_E_LIMIT and a message that names d."""
    import analogy_model as am
    rng = np.random.default_rng(12)
    N = 200
    ids = np.arange(1, N + 1, dtype=np.int32)
    triples = ids[rng.integers(0, N, size=(5, 3))]
    x = rng.standard_normal((N, 3029)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    idx = gpu.VectorIndex(ids, x)
    for method in ("3cosadd", "3cosmul"):
        gi, gs = idx.analogy(triples, k=5, method=method)
        ei, es = am.model(x, ids, triples, 5, method)
        assert np.array_equal(gi, ei) and np.array_equal(gs.view(np.uint64), es.view(np.uint64)), method
    idx.close()
    idx = gpu.VectorIndex(ids[:8], np.ascontiguousarray(np.pad(x[:8], ((0, 0), (0, 1)))))
    for method in ("3cosadd", "3cosmul"):
        with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*d=3030"):
            idx.analogy(triples[:1] % 8 + 1, k=1, method=method)
    idx.close()


# ---------------------------------------------------------------------------------------
# 2. flat PQ and grouping over (d, m, K)
# ---------------------------------------------------------------------------------------
PQ_SHAPES = [(25, 5, 256),      # the shape the reference ships
             (300, 6, 256),     # S = 50
             (300, 15, 128),    # odd m: the last code dword of a row is half filled
             (300, 30, 32),     # M2 = 15
             (64, 8, 16),
             (128, 1, 256),     # m = 1
             (300, 12, 2048),   # K above the fused path's 1024
             (300, 30, 1024),   # 120 KiB LUT, just inside check_pq_shape
             (55, 11, 16),      # odd m with M2 = 6: grouping_kernel<6>
             (58, 29, 16)]      # odd m with M2 = 15: grouping_kernel<15>


def test_pq_shape_list_reaches_every_grouping_instantiation():
    m2 = {(m + 1) // 2: m for _, m, _ in PQ_SHAPES}
    assert 6 in m2 and 15 in m2 and len(set(m2) - {6, 15}) >= 2, m2
    odd = {(m + 1) // 2 for _, m, _ in PQ_SHAPES if m % 2}
    assert 6 in odd and 15 in odd and odd - {6, 15}, odd   # an odd m for <6>, <15> and the generic <0>


def _pq_setup(gpu, oracle, d, m, K, N):
    t = util.shape_pq_tables(d, m, K, N)
    ot = oracle.pq_table(t["codebook"], t["ids"], t["codes"])
    idx = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    return t, ot, idx


@pytest.mark.parametrize("d,m,K", PQ_SHAPES)
def test_pq_search_other_shapes(gpu, oracle, d, m, K):
    """pq_search over a flat PQ table of another shape: pq_use_fused and pq_one_shape are false whatever option pq_fused says,
    the generic lut_build + adc_scan<0, .> + merge run (bigk's selection passes from k = 513 on); one query, a batch below and
    one above the fused path's threshold of 16; a subset with duplicates and unknown ids."""
    N = 6000
    t, ot, idx = _pq_setup(gpu, oracle, d, m, K, N)
    qs = util.shape_queries(N, d, 130)
    for k in (1, 5, 32, 600):
        exp = np.stack([oracle.pq_search(ot, q, k) for q in qs])
        for Q in (1, 17, 130):
            for fused in (1, 0, -1):
                idx.set_option("pq_fused", fused)
                (gi, gd), names = _profiled(idx, lambda: idx.search(qs[:Q], k, sentinel=100.0))
                what = f"pq d={d} m={m} K={K} Q={Q} k={k} pq_fused={fused}"
                util.assert_same_lists(gi, gd, exp[:Q], what)
                assert "adc_scan" in names and "lut_build" in names, (what, sorted(names))
                assert not names & {"pq_front", "pq_one", "ivf_filter"}, (what, sorted(names))
                assert ("bigk_replay" in names) == (k == 600) and ("merge_replay" in names) == (k != 600), (what, sorted(names))
    rng = np.random.default_rng(3)
    targets = rng.choice(np.arange(1, N + 1), size=1500, replace=False).astype(np.int32)
    targets = np.concatenate([targets, targets[:50], np.array([N + 5, -3], np.int32)])
    for Q, k in ((1, 5), (17, 5), (130, 32)):
        (gi, gd), names = _profiled(idx, lambda: idx.search(qs[:Q], k, sentinel=1000.0, subset_ids=targets))
        util.assert_same_lists(gi, gd, oracle.pq_search_in_batch(ot, qs[:Q], k, targets, use_target_lists=True), f"pq subset d={d} m={m} K={K} Q={Q}")
        assert "gather_rows" in names and "adc_scan" in names and "pq_front" not in names, sorted(names)
    gi, gd = idx.search(qs[:2], 7, sentinel=1000.0, subset_ids=targets[:3])   # fewer rows than k: sentinel entries stay
    util.assert_same_lists(gi, gd, np.stack([oracle.pq_search_in(ot, q, 7, targets[:3]) for q in qs[:2]]), "pq subset of three rows")
    idx.close()


@pytest.mark.parametrize("d,m,K", PQ_SHAPES)
def test_grouping_other_shapes(gpu, oracle, d, m, K):
    """grouping_pq: grouping_kernel<6> (M2 = 6), <15> (M2 = 15) and the generic <0>, each also with an odd m, whose last code
    dword holds ONE position.  1, 4 and 37 groups, two of them the same vector (the first of equally near groups wins), the whole
    table and a subset with duplicates and unknown ids."""
    N = 6000
    t, ot, idx = _pq_setup(gpu, oracle, d, m, K, N)
    x = util.shape_corpus(N, d).numpy()
    rng = np.random.default_rng(5)
    sub = np.concatenate([rng.choice(np.arange(1, N + 1), size=900, replace=False).astype(np.int32), np.array([7, 7, N + 3, -2], np.int32)])
    for G in (1, 4, 37):
        gv = x[rng.choice(N, size=G, replace=False)].copy()
        if G > 1:
            gv[G // 2] = gv[0]                      # the same vector twice: group 0 wins every tie against group G // 2
        for s in (None, sub):
            (gi, gg), names = _profiled(idx, lambda: idx.grouping(gv, s))
            ei, eg = oracle.grouping_pq(ot, gv, t["ids"] if s is None else s)
            assert "grouping" in names and "lut_build" in names, sorted(names)
            assert np.array_equal(gi, ei) and np.array_equal(gg, eg), (d, m, K, G, s is None, np.nonzero(gg != eg)[0][:5])
            assert G == 1 or (gg != G // 2).all()
    idx.close()


def test_pq_shape_beyond_the_lut_limit_is_refused(gpu):
    """check_pq_shape: m * K * 4 + 4096 bytes must fit the 160 KiB of LDS; m = 40, K = 1024 (160 KiB of LUT) is refused when pinned."""
    rng = np.random.default_rng(1)
    cb = rng.standard_normal((40, 1024, 1)).astype(np.float32)
    with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT):
        gpu.PQIndex(cb, np.arange(1, 65, dtype=np.int32), np.zeros((64, 40), np.int16))


# ---------------------------------------------------------------------------------------
# 3. kNN-join over (d, m, K, k_coarse)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,K,kc", [(50, 5, 64, 8), (64, 8, 16, 4), (300, 12, 256, 16), (300, 15, 128, 8)])
def test_knn_join_other_shapes(gpu, oracle, d, m, K, kc):
    """ivpq_search_in at other shapes (half = d / 2 of 25, 32 and 150 dimensions; S = 10, 8, 25, 20; odd and even m; 16, 64
    and 256 cells): the three methods, with and without target lists, a round that doubles alpha (few targets, low confidence:
    the oracle says whether one happened) and k * pvf > 1024 (the post verification's selection passes)."""
    N = 8000
    t = util.shape_ivpq_tables(d, m, K, kc, N)
    ot = oracle.ivpq_table(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])
    idx = gpu.IVPQIndex(t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])
    qs = util.shape_queries(N, d, 40, seed=21)
    rng = np.random.default_rng(5)
    targets = rng.choice(np.arange(1, N + 1), size=3000, replace=False).astype(np.int32)
    doubled = False
    for method in (0, 1, 2):
        for use_tl in (True, False):
            for (k, alpha, pvf, T, conf) in [(5, 3, 20, 3000, 0.8), (10, 10, 7, 3000, 0.8), (5, 1, 3, 300, 0.3), (20, 1, 3, 300, 0.05),
                                             (60, 5, 20, 3000, 0.8)]:
                gi, gd, git = idx.knn_join(qs, k, targets[:T], alpha, pvf, method, use_target_lists=use_tl, confidence=conf)
                exp, eit = oracle.ivpq_search_in(ot, qs, k, targets[:T], alpha, pvf, method, use_target_lists=use_tl, confidence=conf)
                assert git == eit, (git, eit)
                doubled |= eit > 1
                util.assert_same_lists(gi, gd, exp, f"join d={d} m={m} K={K} kc={kc} method={method} tl={use_tl} k={k} alpha={alpha} pvf={pvf} T={T}")
    assert doubled, "no case of this shape went into a second round"
    idx.close()


def test_knn_join_odd_d_is_refused(gpu):
    """The coarse multi-index halves the vector: d = 25 has no halves."""
    rng = np.random.default_rng(2)
    with pytest.raises(gpu.FreddyGpuError, match="bad coarse multi-index shape"):
        gpu.IVPQIndex(rng.standard_normal((5, 16, 5)).astype(np.float32), rng.standard_normal((2, 4, 12)).astype(np.float32),
                      np.arange(1, 9, dtype=np.int32), np.zeros(8, np.int32), np.zeros((8, 5), np.int16), None, np.zeros(17, np.float32))


# ---------------------------------------------------------------------------------------
# 4. encode and k-means
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,K", [(16, 16, 32), (25, 5, 256), (160, 8, 64), (300, 6, 256)])
def test_encode_other_sub_vector_sizes(gpu, oracle, d, m, K):
    """S = 1 (d = m), 5, 20, 50: encode_pq_kernel<0, 4>, the instantiation with a runtime S (<25, 4> and <10, 4> are the other
    two).  A duplicated codeword (the lower code wins), an exact hit; coarse quantizers of 1, 63, 65 and 200 cells (one and two
    passes of a wave's 64 lanes, with and without a ragged end), one centroid duplicated."""
    N = 3000
    S = d // m
    x = util.shape_corpus(N, d).numpy()
    rng = np.random.default_rng(K + m)
    cb = (rng.standard_normal((m, K, S)) * 0.05).astype(np.float32)
    cb[0, K - 1] = cb[0, 1]
    cb[m - 1, 5] = x[11, (m - 1) * S:]
    cell, codes = gpu.encode(cb, x)
    assert cell is None
    assert np.array_equal(codes, oracle.encode_pq(cb, x))
    assert codes[11, m - 1] == 5 and (codes[:, 0] != K - 1).all()
    for C in (1, 63, 65, 200):
        coarse = x[rng.choice(N, C, replace=False)].copy()
        if C > 1:
            coarse[C - 1] = coarse[C // 3]
        cell, codes = gpu.encode(cb, x, coarse=coarse)
        exp_cell = oracle.assign_coarse(coarse, x)
        assert np.array_equal(cell, exp_cell) and (C == 1 or (cell != C - 1).all()), C
        res = np.stack([oracle.vec_minus(x[i], coarse[exp_cell[i]]) for i in range(N)])
        assert np.array_equal(codes, oracle.encode_pq(cb, res)), C


def test_encode_crosses_the_chunk_boundary(gpu, oracle):
    """encode_impl works through 65 536 rows at a time: 65 536 + 77 rows (8-d, m = 4: S = 2) -- the second chunk's codes and
    cells land behind the first's."""
    N, d, m, K = 65536 + 77, 8, 4, 16
    x = util.shape_corpus(N, d).numpy()
    rng = np.random.default_rng(9)
    cb = (rng.standard_normal((m, K, d // m)) * 0.3).astype(np.float32)
    cb[1, K - 1] = cb[1, 2]
    coarse = x[[5, 70000 % N, 333]].copy()
    _, codes = gpu.encode(cb, x)
    assert np.array_equal(codes, oracle.encode_pq(cb, x)) and (codes[:, 1] != K - 1).all()
    cell, codes = gpu.encode(cb, x, coarse=coarse)
    exp_cell = oracle.assign_coarse(coarse, x)
    assert np.array_equal(cell, exp_cell)
    res = np.stack([oracle.vec_minus(x[i], coarse[exp_cell[i]]) for i in range(N)])
    assert np.array_equal(codes, oracle.encode_pq(cb, res))
    assert len(np.unique(codes[65536:], axis=0)) > 1


@pytest.mark.parametrize("d", [1, 5, 301, 1024])
def test_kmeans_over_d(gpu, oracle, d):
    """Lloyd k-means at d = 1, 5, 301 (the second of kmeans_update_kernel's four dimension slots half used) and 1024 (all four
    full: the limit): centroids and assignment bit for bit; explicit and default initial rows, one cluster, as many as rows."""
    n = 2000
    x = util.shape_corpus(n, d).numpy() if d > 1 else np.random.default_rng(4).standard_normal((n, 1)).astype(np.float32)
    rng = np.random.default_rng(21 + d)
    for vecs, k, iters, init in ((x, 7, 4, rng.choice(n, 7, replace=False).astype(np.int32)), (x, 1, 2, np.array([n - 1], np.int32)),
                                 (x[:50], 50, 3, rng.permutation(50).astype(np.int32)), (x[:600], 65, 2, None)):
        gc, ga = gpu.kmeans(vecs, k, iters, init)
        oc, oa = oracle.kmeans(vecs, k, iters, init)
        assert np.array_equal(ga, oa), (d, k)
        assert np.array_equal(gc.view(np.uint32), oc.view(np.uint32)), (d, k)


def test_kmeans_beyond_1024_dimensions_is_refused(gpu):
    with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*d=1025"):
        gpu.kmeans(np.zeros((8, 1025), np.float32), 2, 1, np.array([0, 1], np.int32))


# ---------------------------------------------------------------------------------------
# 5. IVFADC above 300 and above 1024 dimensions
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,K,C", [(384, 12, 256, 24), (1200, 12, 16, 8)])
def test_ivfadc_wide_vectors(gpu, oracle, d, m, K, C):
    """d = 384 (S = 32): above the 300 dimensions of the MFMA cell selection (r.approx is off), so batches take the fp32
    coarse_tile_kernel.  d = 1200 (S = 100): above 1024, where the small-batch coarse kernel's 1024-float query buffer does not
    reach -- coarse_dist_kernel<16> with memsets in front (r.zeroed false), 75 KiB of dynamic LDS.
    r.tiled = (Q >= 32): Q = 5 and 31 are small batches, Q = 32 and 100 tiled ones.  Both found rules; option fused -1, 1, 0:
    ivf_multi_kernel when forced (and unforced from 256 (query, cell) items on), lut_build + adc_scan when switched off -- never
    the m = 12 / S = 25 filter scan."""
    N = 8000
    t = util.shape_ivf_tables(d, m, K, C, N)
    ot = oracle.ivf_table(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    qs = util.shape_queries(N, d, 100, seed=3)
    for k, W, rule, sent in ((5, 3, 0, 1000.0), (10, 2, 1, 100.0)):
        exp = oracle.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule)
        for Q in (5, 31, 32, 100):
            for fused in (-1, 1, 0):
                idx.set_option("fused", fused)
                (gi, gd), names = _profiled(idx, lambda: idx.search(qs[:Q], k, W, sentinel=sent, found_rule=rule))
                what = f"ivfadc d={d} Q={Q} k={k} W={W} rule={rule} fused={fused}"
                util.assert_same_lists(gi, gd, exp[:Q], what)
                assert "coarse_dist" in names and not names & {"ivf_filter", "ivf_one", "coarse_table"}, (what, sorted(names))
                if fused == 1 or (fused == -1 and Q * W >= 256):
                    assert "ivf_multi_scan" in names and "adc_scan" not in names, (what, sorted(names))
                else:
                    assert "adc_scan" in names and "lut_build" in names and "ivf_multi_scan" not in names, (what, sorted(names))
    idx.close()


def test_ivfadc_beyond_2560_dimensions_is_refused(gpu):
    """coarse_dist_kernel<16> keeps 16 queries of d floats in LDS: 160 KiB at d = 2560; freddy_gpu_pin_ivf refuses more."""
    rng = np.random.default_rng(3)
    d = 2564
    with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*d=2564"):
        gpu.IVFIndex(rng.standard_normal((2, d)).astype(np.float32), rng.standard_normal((4, 8, d // 4)).astype(np.float32),
                     np.array([0, 4, 8], np.int32), np.arange(1, 9, dtype=np.int32), np.zeros((8, 4), np.int16))
