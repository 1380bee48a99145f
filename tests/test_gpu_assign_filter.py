"""-m gpu tests of option assign_filter (csrc/assign_filter.h): freddy_gpu_exact_assign and freddy_gpu_cluster as matrix-core filter +
exact refine + redo.  Every output is compared bit for bit with the numpy model of tests/assign_model.py (or, for the whole k-means,
with the option off); the stats and the profile say which path answered.  "No redo" is asserted only where a condition computed here
from the inputs rules the redo out: the documented eps = rel(d) |x| max|q| + 2e-34 puts a centroid on the device's list only if its
fp64 similarity is within 4 eps of the best one (|a - s| <= eps on both sides of a 2 eps window), and a list of at most KEEP = 16 at
every boundary of 128 centroids is never sent back."""
import numpy as np
import pytest

import assign_model as am
import util

pytestmark = pytest.mark.gpu

KEEP, TILE = 16, 128                  # csrc/encode_filter.h ENC_KEEP; centroids per streamed tile


def eps_rel(d):                        # csrc/assign_filter.h asf_eps_rel
    return 2.5e-5 if d <= 64 else 9e-5 if d <= 320 else 1.4e-4


def crowded(rows, qs):
    """Per row: may more than KEEP centroids lie inside the bracket at some tile boundary?  From the inputs alone."""
    x, q = rows.astype(np.float64), qs.astype(np.float64)
    s = x @ q.T
    eps = eps_rel(x.shape[1]) * np.linalg.norm(x, axis=1) * np.linalg.norm(q, axis=1).max() + 2e-34
    out = np.zeros(len(x), bool)
    for b in list(range(TILE, q.shape[0], TILE)) + [q.shape[0]]:
        out |= (s[:, :b] >= s[:, :b].max(axis=1, keepdims=True) - 4 * eps[:, None]).sum(axis=1) > KEEP
    return out


def make(d, n0=1500, Q=129, n=1000, seed=0):
    """A table of n0 rows, Q centroids that are means of rows (two identical pairs), n targets with ids without a row, duplicated ids
    and duplicated rows."""
    x = util.shape_corpus(n0, d).numpy().copy()
    x[700:720] = x[100:120]
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    rng = np.random.default_rng(97 + d + seed)
    qs = np.stack([x[rng.choice(n0, 10)].mean(axis=0) for _ in range(Q)]).astype(np.float32)
    if Q > 16:
        qs[4] = qs[0]; qs[16] = qs[3]
    tg = rng.choice(ids, n).astype(np.int32)
    if n > 40:
        tg[3] = tg[1]; tg[5] = n0 + 7; tg[30] = -4; tg[31] = 2**31 - 1
        tg[10:20] = np.arange(101, 111); tg[20:30] = np.arange(701, 711)
    return x, ids, qs, tg


def filtered_vec(ids, x):
    from freddy_amd import gpu
    vec = gpu.VectorIndex(ids, x)
    vec.set_option("assign_filter", 1)
    return vec


def test_option_belongs_to_a_vector_handle():
    from freddy_amd import gpu
    x, ids, _, _ = make(30, n0=800, Q=1, n=1)
    vec = gpu.VectorIndex(ids, x)
    vec.set_option("assign_filter", 1)                      # ("unknown option" without the feature)
    vec.set_option("assign_filter", 0)
    pqt = util.shape_pq_tables(25, 5, 256, 2000)
    pq = gpu.PQIndex(pqt["codebook"], pqt["ids"], pqt["codes"])
    with pytest.raises(gpu.FreddyGpuError, match="error -4"):
        pq.set_option("assign_filter", 1)
    vec.close(); pq.close()


@pytest.mark.parametrize("d", [7, 30, 32, 33, 300, 512])
def test_filter_equals_the_model(d):
    x, ids, qs, tg = make(d)
    assert not crowded(x[tg[am.rows_of(ids, tg) >= 0] - 1], qs).any()
    vec = filtered_vec(ids, x)
    vec.profile_enable(True)
    for Q in (1, 17, 33, 129):
        for n in (1, 63, 64, 65, 1000):
            got, exp = vec.assign(qs[:Q], tg[:n]), am.exact_assign(ids, x, qs[:Q], tg[:n])
            assert am.same(got, exp), f"d={d} Q={Q} n={n}: {np.flatnonzero(got[0] != exp[0])[:8]}"
            st = vec.last_assign_stats()
            assert st["filtered"] == (am.rows_of(ids, tg[:n]) >= 0).sum() and st["redone"] == 0 and st["candidates"] >= st["filtered"], (Q, n, st)
    q = got[0]
    assert q[5] == -1 and q[30] == -1 and q[31] == -1 and q[3] == q[1] and np.array_equal(q[10:20], q[20:30])
    assert not np.isin(q, [4, 16]).any(), "the later of two identical centroids won a target"
    names = set(vec.profile_read())
    assert {"assign_image_kernel", "assign_filter_kernel", "assign_refine_kernel"} <= names and "assign_exact_kernel" not in names, names
    vec.close()


def test_wider_than_the_bracket_takes_the_exact_kernel():
    x, ids, qs, tg = make(513, n0=800, Q=17, n=65)
    vec = filtered_vec(ids, x)
    vec.profile_enable(True)
    assert am.same(vec.assign(qs, tg), am.exact_assign(ids, x, qs, tg))
    assert set(vec.profile_read()) == {"assign_exact_kernel"} and vec.last_assign_stats()["filtered"] == 0
    vec.close()


@pytest.mark.parametrize("case", ["ties", "nan", "neg_nan", "pos_inf", "both_inf", "bad_rows", "tiny", "huge"])
def test_redo_paths(case):
    """40 identical centroids (more ties than a list keeps), a poisoned centroid (the image's flag: every target), rows with NaN / +Inf /
    -Inf (those targets only), and everything scaled by 2^-60 / 2^60 (subnormal or very large products: whichever path).  Then a
    healthy call on the same handle."""
    d = 300
    x, ids, qs, tg = make(d, n0=800, Q=33, n=200, seed=1)
    healthy_qs = qs.copy()
    have = am.rows_of(ids, tg) >= 0
    assert not crowded(x[tg[have] - 1], qs).any()
    bad_rows = np.array([7, 64, 65])
    if case == "ties":
        qs = np.repeat(qs[:1], 40, axis=0)
    elif case == "bad_rows":
        x[7, 3] = np.nan; x[64, d - 1] = np.inf; x[65, 0] = -np.inf
        tg[40:43] = bad_rows + 1
    elif case in ("tiny", "huge"):
        f = np.float32(2.0 ** (-60 if case == "tiny" else 60))
        x, qs, healthy_qs = x * f, qs * f, healthy_qs * f
    else:
        qs[9] = util.poison_query(qs[9], case, 1, np.random.default_rng(3))
    vec = filtered_vec(ids, x)
    got = vec.assign(qs, tg)
    st = vec.last_assign_stats()
    assert am.same(got, am.exact_assign(ids, x, qs, tg)), np.flatnonzero(got[0] != am.exact_assign(ids, x, qs, tg)[0])[:8]
    assert st["filtered"] == have.sum()
    if case == "ties":
        assert st["redone"] == have.sum() > 0 and (got[0][have] == 0).all()
    elif case == "bad_rows":
        is_bad = np.isin(am.rows_of(ids, tg), bad_rows)
        assert not crowded(x[tg[have & ~is_bad] - 1], qs).any()
        assert st["redone"] == is_bad.sum() >= 3
    elif case not in ("tiny", "huge"):
        assert st["redone"] == have.sum()
        if case in ("nan", "neg_nan"):
            assert (got[0][have] == 9).all() and np.isnan(got[1][have]).all()
    assert am.same(vec.assign(healthy_qs, tg), am.exact_assign(ids, x, healthy_qs, tg))
    if case in ("ties", "nan", "neg_nan", "pos_inf", "both_inf"):
        assert vec.last_assign_stats()["redone"] == 0
    vec.close()


def test_self_check_compares_every_bracket():
    x, ids, qs, tg = make(300, Q=129, n=300)
    vec = filtered_vec(ids, x)
    exp = vec.assign(qs, tg)
    vec.set_option("check_brackets", 16)
    before = (vec.lib.freddy_gpu_filter_bound_checked(vec.h), vec.lib.freddy_gpu_filter_bound_violations(vec.h))
    got = vec.assign(qs, tg)
    st = vec.last_assign_stats()
    n_rows = int((am.rows_of(ids, tg) >= 0).sum())
    assert am.same(got, exp) and am.same(got, am.exact_assign(ids, x, qs, tg))
    assert st["violations"] == 0 and st["checked"] == n_rows * 129 and st["redone"] == 0, st
    assert vec.lib.freddy_gpu_filter_bound_checked(vec.h) - before[0] == n_rows * 129
    assert vec.lib.freddy_gpu_filter_bound_violations(vec.h) == before[1]
    vec.close()


@pytest.mark.parametrize("n,kc,option", [(90, 7, None), (90, 40, None), (5000, 7, None), (5000, 40, None),
                                         (5000, 7, ("cluster_pass", 64)), (5000, 40, ("grid_cus", 1))])
def test_whole_kmeans_equals_the_option_off(n, kc, option):
    from freddy_amd import gpu
    x = util.corpus(8000).numpy()
    ids = np.arange(1, 8001, dtype=np.int32)
    rng = np.random.default_rng(n + kc)
    tokens = np.sort(rng.choice(ids, n, replace=False)).astype(np.int32)
    draws = rng.random(kc + 9 * kc * 10)
    vec = gpu.VectorIndex(ids, x)
    if option:
        vec.set_option(*option)
    off = vec.cluster(tokens, kc, draws)
    vec.set_option("assign_filter", 1)
    vec.profile_enable(True)
    on = vec.cluster(tokens, kc, draws)
    names = set(vec.profile_read())
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1].view(np.uint32), off[1].view(np.uint32))
    assert np.array_equal(on[2].view(np.uint32), off[2].view(np.uint32))
    assert "assign_filter_kernel" in names and "assign_exact_kernel" not in names, names
    assert vec.last_assign_stats()["filtered"] == 10 * n
    vec.close()
