"""Option exact_wide: exact kNN as filter + refine for tables of 512 < d <= 2048 (csrc/exact_wide.h streams the query image
through LDS; exact2.h: the bracket for the longer chain).  Every list is compared bit for bit with the oracle's exact_knn."""
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


def _table(d, N, scale=1.0):
    """test_gpu_shapes._exact_table: duplicate rows, 70 queries, a negated one and one with copies in the table."""
    x = (util.shape_corpus(N, d).numpy() * np.float32(scale)).astype(np.float32)
    x[N // 2:N // 2 + 40] = x[100:140]
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    qs = x[::N // 70][:70].copy()
    qs[3] = -qs[3]
    qs[6] = x[100]
    return x, ids, qs


def _wide(gpu, ids, x, **options):
    idx = gpu.VectorIndex(ids, x)
    idx.set_option("exact_wide", 1)
    for name, value in options.items():
        idx.set_option(name, value)
    return idx


def _search(idx, qs, k):
    """(ids, similarities, names of the kernels launched)"""
    idx.profile_enable(True)
    gi, gs = idx.search(qs, k)
    names = set(idx.profile_read())
    idx.profile_enable(False)
    return gi, gs, names


def _refine_all(gpu, oracle, x, ids, qs, what):
    """check_brackets = 4: every (query, row) pair is refined and compared with its bracket.  -> the ids found"""
    idx = _wide(gpu, ids, x, check_brackets=4)
    gi, gs, names = _search(idx, qs, 5)
    assert "exact_filter_wide" in names and "exact_scan" not in names, sorted(names)
    assert idx.bound_violations() == 0
    assert idx.bound_checked() == qs.shape[0] * x.shape[0]
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, q, 5) for q in qs], 5, what)
    idx.close()
    return gi


@pytest.mark.parametrize("d", [516, 768, 1024, 2048])
def test_wide_lists_and_path(gpu, oracle, d):
    """T = 33 (a short last segment), 48, 64, 128; 258 strips (no multiple of 8); Q = 1, 9 (one tile), 70 (two passes, the second
    of 6 queries); d = 1024 again on a grid of 6 workgroups: six rounds, the last with idle waves and idle workgroups."""
    x, ids, qs = _table(d, 8192 + 40)
    exp = [oracle.exact_knn(x, ids, q, 32) for q in qs]
    idx = _wide(gpu, ids, x)
    for cus in (0, 3) if d == 1024 else (0,):
        idx.set_option("grid_cus", cus)
        for Q in (1, 9, 70):
            for k in (1, 5, 32):
                gi, gs, names = _search(idx, qs[:Q], k)
                util.assert_exact_lists(gi, gs, exp, k, f"d={d} Q={Q} k={k} grid_cus={cus}")
                assert {"exact_filter_wide", "exact_refine"} <= names and "exact_scan" not in names, (d, Q, k, sorted(names))
    assert idx.bound_violations() == 0
    idx.close()


@pytest.mark.parametrize("d,scale", [(516, 1.0), (2048, 1.0), (2048, 3000.0), (2048, 2e-4)])
def test_wide_bracket_holds_for_every_row(gpu, oracle, d, scale):
    N = 8192 + 77
    x, ids, qs = _table(d, N, scale)
    x[1000:1040] *= np.float32(37.5)                # a few long rows: the norm bound is their norm
    x[2000:2020] = 0.0
    rng = np.random.default_rng(d)
    qs = np.concatenate([qs[:10], (rng.standard_normal((2, d)) * 0.01 * scale).astype(np.float32)])
    _refine_all(gpu, oracle, x, ids, qs, f"every row d={d} scale={scale}")


def test_wide_bracket_at_the_worst_rounding_of_the_chain(gpu, oracle):
    """x = q = (1, t, ..., t), t * t just below (above) half an ulp of 1: all 2047 additions round one way, the chain returns 1
    (1 + 2047 * 2^-23) while the product is 1 + 2047 t^2 -- more than 1.2e-4 |x||q| apart, the term exf_eps_factor grows for."""
    d, N = 2048, 8192 + 13
    x, ids, qs = _table(d, N)
    lo, hi = np.float32(np.sqrt(0.999 * 2.0 ** -24)), np.float32(np.sqrt(1.001 * 2.0 ** -24))
    down = np.full(d, lo, np.float32); down[0] = 1.0
    up = np.full(d, hi, np.float32); up[0] = 1.0
    assert oracle.cosine_similarity_bytea(down, down) == np.float32(1.0)
    assert oracle.cosine_similarity_bytea(up, up) == np.float32(1.0 + 2047 * 2.0 ** -23)
    for v in (down, up):
        true = float(np.dot(v.astype(np.float64), v.astype(np.float64)))
        gap = abs(float(oracle.cosine_similarity_bytea(v, v)) - true)
        assert gap > 1.2e-4 * true, gap
    x[4000], x[4001], x[4002], x[4003] = down, up, -down, -up
    gi = _refine_all(gpu, oracle, x, ids, np.stack([down, up, -down, -up, qs[0], qs[3]]), "worst rounding of the chain")
    assert gi[0, 0] in (ids[4000], ids[4001]) and gi[2, 0] in (ids[4002], ids[4003])


def test_wide_raised_floor_when_the_unscale_underflows(gpu, oracle):
    """Table at 2^-70, queries at 2^-60: eq + ex >= 150, qunscale = 0, every approximate value is 0 and eps(q) rests on its floor,
    which is d 2^-122 rounded up: 4e-34 at d = 2048 (1e-34 would be below |s| there)."""
    d = 2048
    x, ids, qs = _table(d, 8192 + 5)
    x, qs = np.ldexp(x, -70).astype(np.float32), np.ldexp(qs[:6], -60).astype(np.float32)
    ex = 14 - int(np.frexp(np.abs(x).max())[1])     # exf_scale_exp: the largest |element| lands in [2^13, 2^14)
    eq = [14 - int(np.frexp(np.abs(q).max())[1]) for q in qs]
    assert min(eq) + ex >= 150, (ex, eq)
    _refine_all(gpu, oracle, x, ids, qs, "eq + ex >= 150")


def test_wide_state(gpu, oracle):
    d, N0, N1 = 768, 8192 + 8, 8192 + 8 + 45
    x, ids, qs = _table(d, N1)
    x[N0 + 5] *= np.float32(300.0)                  # the append brings a larger element: the copy is laid out again
    qs = np.concatenate([qs[:9], x[N0 + 5:N0 + 6]])
    idx = gpu.VectorIndex(ids[:N0], x[:N0])
    before = idx.nbytes
    idx.set_option("exact_wide", 1)
    assert idx.nbytes - before >= N0 * d * 4
    idx.set_option("exact_wide", 0)
    assert idx.nbytes == before and "exact_scan" in _search(idx, qs, 5)[2]
    join_before = _search_join(idx, qs, ids[:N0])
    idx.set_option("exact_wide", 1)
    assert N0 % 32
    idx.append_rows(ids[N0:], vectors=x[N0:])
    gi, gs, names = _search(idx, qs, 5)
    assert "exact_filter_wide" in names and "exact_scan" not in names, sorted(names)
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x, ids, q, 5) for q in qs], 5, "after the append")
    assert _search_join(idx, qs, ids[:N0]) == join_before
    assert idx.bound_violations() == 0
    idx.close()
    rng = np.random.default_rng(3)
    x2 = rng.standard_normal((300, 2052)).astype(np.float32)
    idx = gpu.VectorIndex(ids[:300], x2)
    with pytest.raises(gpu.FreddyGpuError, match=E_LIMIT + r".*d=2052"):
        idx.set_option("exact_wide", 1)
    gi, gs, names = _search(idx, x2[:3], 5)
    assert "exact_scan" in names
    util.assert_exact_lists(gi, gs, [oracle.exact_knn(x2, ids[:300], q, 5) for q in x2[:3]], 5, "d=2052 after the refusal")
    idx.close()


def _search_join(idx, qs, targets):
    """the kernel names exact_join launches over `targets`"""
    idx.profile_enable(True)
    idx.join(qs, 5, targets)
    names = sorted(idx.profile_read())
    idx.profile_enable(False)
    return names
