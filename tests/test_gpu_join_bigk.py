"""-m gpu: the kNN-join (freddy_gpu_knn_join, the body of ivpq_search_in) with method 0 (ADC) and method 1 (exact) at
512 < k <= 4096: the 2k smallest keys of a query selected 1024 per pass (join_query_kernel<16, true>) and the list written in
closed form by bigk_replay_kernel.  Ids, ranks, distance bits and iteration counts are the oracle's.  The inputs
(tests/join_bigk_inputs.py) tie most queries across the k-th place; tests/test_join_bigk_inputs_cpu.py proves that."""
import numpy as np
import pytest

import join_bigk_inputs as jb
import util
from test_gpu_udf import _cluster_reference, _sim_of, db, same  # noqa: F401  (db: that module's session fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


@pytest.fixture(scope="module")
def idx(gpu):
    ix = gpu.IVPQIndex(*jb.pin_args())
    yield ix
    ix.close()


def check(idx, oracle, method, k, alpha, nt, conf, use_tl=True, double_threshold=10000000):
    gi, gd, git = idx.knn_join(jb.queries(), k, jb.targets(nt), alpha, jb.PVF, method, use_target_lists=use_tl, confidence=conf,
                               double_threshold=double_threshold)
    exp, eit = jb.expected(oracle, method, k, alpha, nt, conf, use_tl, double_threshold)
    what = f"knn_join method={method} k={k} alpha={alpha} targets={nt} conf={conf} tl={use_tl} dt={double_threshold}"
    assert git == eit, (what, git, eit)
    util.assert_same_lists(gi, gd, exp, what)
    return exp, eit


@pytest.mark.parametrize("use_tl", [True, False])
@pytest.mark.parametrize("method", jb.METHODS)
def test_lists_beyond_512_entries_match_the_oracle(idx, oracle, method, use_tl):
    rounds = []
    for (k, alpha, nt, conf) in jb.CASES:
        exp, it = check(idx, oracle, method, k, alpha, nt, conf, use_tl)
        rounds.append(it)
        if nt is not None and nt < k:   # fewer targets than slots: the rest stays (-1, 1000.0)
            assert ((exp["id"] >= 0).sum(1) == nt).all()
    if use_tl:
        assert rounds == [1, 2, 1, 2, 2, 1], rounds


def test_pair_codes(idx, oracle):
    check(idx, oracle, 0, 600, 1, None, 0.8, double_threshold=20)


@pytest.mark.parametrize("method", jb.METHODS)
def test_targets_with_duplicates_and_an_unknown_id(idx, oracle, method):
    tg = jb.odd_targets()
    gi, gd, git = idx.knn_join(jb.queries(), 600, tg, 2, jb.PVF, method)
    exp, eit = oracle.ivpq_search_in(jb.oracle_table(oracle), jb.queries(), 600, tg, 2, jb.PVF, method)
    assert git == eit
    util.assert_same_lists(gi, gd, exp, f"odd targets method={method}")


def test_host_traversal_scans_behind_the_device_part(gpu, oracle):
    """Every traversal on the host heap: the scan list's host-traversed part (flat cell lists, a join launch of its own)."""
    ix = gpu.IVPQIndex(*jb.pin_args())
    ix.set_option("join_host_traversal", 1)
    for method in jb.METHODS:
        check(ix, oracle, method, 600, 1, None, 0.8)
    ix.close()


def test_the_old_path_is_the_old_path(idx, oracle):
    """k = 5 and k = 512 (methods 0, 1, 2) and method 2 with k * pvf = 2000 before and after a k = 4096 call on one handle: the big
    call leaves no workspace or LDS plan behind that the calls below the threshold read."""
    ot, qs = jb.oracle_table(oracle), jb.queries()
    small = [(m, k, 3, 4) for m in (0, 1, 2) for k in (5, 512)] + [(2, 100, 30, 20)]
    want = {c: oracle.ivpq_search_in(ot, qs, c[1], jb.targets(), c[2], c[3], c[0]) for c in small}

    def old_path(when):
        for c in small:
            method, k, alpha, pvf = c
            gi, gd, git = idx.knn_join(qs, k, jb.targets(), alpha, pvf, method)
            assert git == want[c][1], (when, c)
            util.assert_same_lists(gi, gd, want[c][0], f"{when} the k = 4096 call: method={method} k={k} alpha={alpha} pvf={pvf}")

    old_path("before")
    for method in jb.METHODS:
        check(idx, oracle, method, 4096, 1, None, 0.8)
        old_path("after")


def test_limits(gpu, idx, oracle):
    qs, tg = jb.queries(), jb.targets()
    for method in jb.METHODS:
        with pytest.raises(gpu.FreddyGpuError, match=r"freddy_gpu error -5.*k=4097") as e:
            idx.knn_join(qs, 4097, tg, 1, jb.PVF, method)
        assert "hip" not in str(e.value).lower()
    with pytest.raises(gpu.FreddyGpuError, match=r"freddy_gpu error -5.*k\*pvf=8194") as e:
        idx.knn_join(qs, 4097, tg, 1, 2, 2)
    assert "hip" not in str(e.value).lower()
    for method in (0, 1, 2):
        gi, gd, git = idx.knn_join(qs, 5, tg, 3, 4, method)
        exp, eit = oracle.ivpq_search_in(jb.oracle_table(oracle), qs, 5, tg, 3, 4, method)
        assert git == eit
        util.assert_same_lists(gi, gd, exp, f"k = 5 after the refused calls, method={method}")


@pytest.mark.parametrize("method", jb.METHODS)
def test_nonfinite_queries(idx, oracle, method):
    """A NaN and an Inf query among healthy ones: the oracle's lists for all, and the healthy queries' lists are those of the call
    without the poisoned ones."""
    k, alpha, conf = jb.NONFINITE_CASE
    qs, mask = jb.poisoned_queries()
    gi, gd, git = idx.knn_join(qs, k, jb.targets(), alpha, jb.PVF, method, confidence=conf)
    exp, eit = oracle.ivpq_search_in(jb.oracle_table(oracle), qs, k, jb.targets(), alpha, jb.PVF, method, confidence=conf)
    assert git == eit
    util.assert_same_lists(gi, gd, exp, f"poisoned queries method={method}")
    hi, hd, _ = idx.knn_join(jb.queries(), k, jb.targets(), alpha, jb.PVF, method, confidence=conf)
    assert np.array_equal(gi[~mask], hi[~mask]) and np.array_equal(gd[~mask].view(np.uint32), hd[~mask].view(np.uint32))
    assert (gi[mask] == -1).all() and (gd[mask] == np.float32(1000.0)).all()


def test_cluster_ivpq_over_1000_tokens(db, oracle):
    """cluster_ivpq asks the join for all n tokens per centroid (k = n): 1000 tokens at the SQL default method_flag = 0."""
    s, t = db
    x = t["x"]
    N = x.shape[0]
    rng = np.random.default_rng(33)
    tokens = np.sort(rng.choice(np.arange(1, N + 1), 1000, replace=False)).astype(np.int32)
    vecs = x[tokens - 1]
    k, n = 7, len(tokens)
    draws = rng.random(k + 9 * k * 10)
    s.set_alpha(3); s.set_pvf(4); s.set_method_flag(0)

    def rows_ivpq(cent):
        e, _ = oracle.ivpq_search_in(t["ivpq"], cent, n, tokens, 3, 4, 0)
        e = e.reshape(len(cent), n)
        return [(_sim_of(oracle, e["dist"][qi, r]), qi + 1, int(np.searchsorted(tokens, e["id"][qi, r])) + 1)
                for qi in range(len(cent)) for r in range(n) if e["id"][qi, r] >= 0]

    exp = _cluster_reference(rows_ivpq, vecs, n, k, draws)
    got = s.cluster_ivpq(tokens, k, draws)
    s.set_pvf(20)
    assert np.array_equal(got, exp), f"cluster_ivpq: {np.flatnonzero(got != exp)[:10]}"


def test_session_knn_join_at_k_600(db, oracle):
    s, t = db
    N = t["x"].shape[0]
    qids = np.arange(100, 108, dtype=np.int32)
    qs = t["x"][qids - 1]
    targets = np.random.default_rng(3).choice(np.arange(1, N + 1), 3000, replace=False).astype(np.int32)
    exp, _ = oracle.ivpq_search_in(t["ivpq"], qs, 600, targets, 3, 4, 0)
    s.set_alpha(3); s.set_pvf(4); s.set_method_flag(0)
    rows = s.knn_join(qs, qids, 600, targets)
    s.set_pvf(20)
    same(rows, exp)
