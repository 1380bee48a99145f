"""No GPU: what tests/test_gpu_assign_filter_edges.py assumes about the inputs of tests/assign_filter_inputs.py, proven from the inputs
alone -- the gap bins of the near-tie groups, "not crowded" wherever the GPU suite asserts redone == 0, the top separation wherever
it asserts redone == predicted_redo().sum(), the scale exponents of the scale-edge cases, and the two properties of the k-means
inputs (a redo in round one of the three-vector tokens; flagged and unflagged rounds for the chosen seed of the NaN tokens)."""
import numpy as np
import pytest

import assign_filter_inputs as fi
import assign_model as am


def test_the_predictor_on_hand_made_lists():
    """predicted_redo against lists written out by hand: d = 2, target (1, 0), similarity = the centroid's first element."""
    x = np.array([[1.0, 0.0]], np.float32)
    q = np.zeros((300, 2), np.float32)
    q[:, 0] = -1.0 - np.arange(300) * 0.01
    for plateau, redo in ((list(range(5, 21)), False), (list(range(5, 22)), True), (list(range(120, 136)), False), (list(range(120, 137)), True),   # 8 + 8, 8 + 9 over a boundary
                          (list(range(120, 128)) + list(range(200, 209)), True), (list(range(256, 273)), True)):
        qq = q.copy(); qq[plateau, 0] = 1.0
        assert fi.top_separated(x, qq).all() and bool(fi.predicted_redo(x, qq)[0]) == redo, plateau
    qq = q.copy(); qq[0:17, 0] = 0.5; qq[130:140, 0] = 1.0       # the 17 are the prefix maximum at the first boundary
    assert fi.predicted_redo(x, qq)[0]
    qq = q.copy(); qq[0:12, 0] = 0.5; qq[130:140, 0] = 1.0       # a compaction that succeeds
    assert not fi.predicted_redo(x, qq)[0]
    qq[7, 1] = np.inf
    assert fi.predicted_redo(x, qq)[0] and fi.image_flag(qq) == (True, 0)
    assert [int(fi.scale_exp(v)) for v in (1.0, 0.99, 2.0 ** 127, 2.0 ** -107, 0.0)] == [13, 14, -114, 120, 0]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("d", fi.DIMS)
def test_near_tie_groups(d, wide):
    x, ids, qs, tg, probes, groups = fi.near_ties(d, wide)
    s, eps = fi.sims64(x[probes], qs), fi.eps_of(x[probes], qs)
    orders = set()
    for p in range(fi.N_PROBES):
        g = s[p, groups[p]]
        gap = (g.max() - g) / eps[p]
        for k, (lo, hi) in enumerate(fi.BINS):
            assert lo <= gap[k] <= hi, (d, wide, p, k, gap)
        assert gap[0] == 0.0 and gap[1] > 0.0, (p, gap[:2])
        rest = np.delete(s[p], groups[p])
        assert (rest <= g.max() - 8 * eps[p]).all(), (d, p, ((g.max() - rest) / eps[p]).min())
        orders.add(bool(groups[p, 0] < groups[p, 1]))
    assert orders == {True, False}, "the two closest of a group come in one index order only"
    assert (groups[:, 0] < fi.TILE).any() and (groups[:, 0] >= fi.TILE).any(), "groups in one tile only"
    have, rows = fi.target_rows(ids, x, tg)
    assert not fi.crowded(rows, qs).any() and not fi.scale_redo(rows, qs).any() and 0 < (~have).sum() < 5
    if wide:                            # the span of the elements of a row and of a centroid
        span = lambda v: np.log2(np.abs(v).max(axis=1) / np.where(v == 0, np.inf, np.abs(v)).min(axis=1))
        assert np.median(span(x)) >= 12 and np.median(span(qs)) >= 12


@pytest.mark.parametrize("d", fi.DIMS)
def test_cancellation(d):
    x, ids, qs, tg = fi.cancellation(d)
    s, eps = fi.sims64(x, qs), fi.eps_of(x, qs)
    assert qs.shape[0] <= fi.KEEP and (np.abs(s) <= 6 * eps[:, None]).mean() > 0.9 and (s > 0).any() and (s < 0).any()
    P = np.abs(x.astype(np.float64)) @ np.abs(qs.astype(np.float64)).T
    assert (P >= 0.95 * np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(qs, axis=1)[None]).all()
    assert not fi.scale_redo(x, qs).any()


@pytest.mark.parametrize("Q", [1, 127, 129, 257])
def test_all_negative(Q):
    x, ids, qs, tg = fi.all_negative(30, Q)
    have, rows = fi.target_rows(ids, x, tg)
    assert have.sum() >= 65 and (~have).sum() == 1 and (fi.sims64(rows, qs) < 0).all()
    assert fi.top_separated(rows, qs).all() and not fi.predicted_redo(rows, qs).any()
    assert (am.exact_assign(ids, x, qs, tg)[0][have] >= 0).all()


def test_zero_cases():
    for name, (x, ids, qs, tg, winner) in fi.zero_cases().items():
        have, rows = fi.target_rows(ids, x, tg)
        assert have.all() and fi.top_separated(rows, qs).all(), name
        pred = fi.predicted_redo(rows, qs)
        zero = ~rows.any(axis=1)
        assert zero.sum() == 1 and zero[0] if name != "all_zero_centroids" else zero.sum() == 1
        assert pred[zero].all() == (name in ("zero_row_Q17", "zero_centroid")) and not pred[~zero].any(), name
        assert (am.exact_assign(ids, x, qs, tg)[0][zero] == winner).all()
        if name == "all_zero_centroids":
            assert (am.exact_assign(ids, x, qs, tg)[0] == 0).all()


def test_scale_cases():
    """e and ec as the kernels derive them, and the rule: a row out of range redoes that target, a centroid scale out of range every
    target, a sum out of range that target."""
    cases = fi.scale_cases()
    exps = {}
    for name, (x, ids, qs, tg) in cases.items():
        have, rows = fi.target_rows(ids, x, tg)
        assert have.all() and qs.shape[0] <= fi.KEEP and fi.margin_ok(rows, qs), name
        flag, ec = fi.image_flag(qs)
        ec_raw = int(fi.scale_exp(np.abs(qs).max()))
        e = fi.scale_exp(np.abs(rows).max(axis=1))
        exps[name] = (ec_raw, [int(v) for v in e[:5]])
    assert exps["rows"] == (0, [120, 121, -114, 119, -113])
    x, ids, qs, tg = cases["rows"]
    assert list(fi.scale_redo(x, qs)[:5]) == [False, True, True, False, True] and not fi.scale_redo(x, qs)[5:].any()
    assert exps["centroids_120"][0] == 120 and exps["centroids_120"][1][:4] == [0, 1, -1, -40]
    x, ids, qs, tg = cases["centroids_120"]
    assert list(fi.scale_redo(x, qs)[:4]) == [False, True, False, False] and fi.scale_redo(x, qs)[4:].all()
    assert exps["centroids_121"][0] == 121 and fi.scale_redo(*cases["centroids_121"][0:3:2]).all()
    assert exps["centroids_-111"][0] == -111 and exps["centroids_-111"][1][:2] == [100, 20]
    x, ids, qs, tg = cases["centroids_-111"]
    assert not fi.scale_redo(x, qs)[0] and fi.scale_redo(x, qs)[1:].all()
    assert exps["centroids_-114"][0] == -114 and fi.scale_redo(*cases["centroids_-114"][0:3:2]).all()   # (max|q| > binary32's range)
    assert exps["sum_120_121"] == (60, [60, 61, 59]) and list(fi.scale_redo(*cases["sum_120_121"][0:3:2])[:3]) == [False, True, False]
    assert exps["sum_-120_-121"] == (-60, [-60, -61, -59]) and fi.scale_redo(*cases["sum_-120_-121"][0:3:2])[:3].all()


@pytest.mark.parametrize("Q", fi.B_QS)
def test_list_cases(Q):
    cases = fi.list_cases(Q)
    assert len(cases) >= 14
    for name, (x, ids, qs, tg, pos, winner, redone) in cases.items():
        assert qs.shape == (Q, fi.B_D) and tg.size == fi.B_N, name
        have, rows = fi.target_rows(ids, x, tg)
        assert (~have).sum() == 1 and fi.top_separated(rows, qs).all() and not fi.scale_redo(rows, qs).any(), name
        pred = np.zeros(tg.size, bool)
        pred[have] = fi.predicted_redo(rows, qs)
        assert (pred[pos] == redone).all(), name
        assert pred.sum() == (len(pos) if redone else 0), (name, pred.sum())    # the planted targets and no other
        assert np.array_equal(am.exact_assign(ids, x, qs, tg)[0][pos], winner), name
        if name.startswith("redo_"):
            cnt, first = int(name.split("_")[1]), int(name.split("_")[3])
            assert pred.sum() == cnt and pos[0] == first and (first < 64 or (pos >= 64).all())


def test_pass_cases():
    for n, a, b, first in ((fi.AS_PASS + 65, 100, 3, fi.AS_PASS), ((1 << 20) + 65, 100, 3, fi.check_pass(17))):
        assert first == min(fi.AS_PASS, first) and first < n <= 2 * first            # two passes
        x, ids, qs, tg = fi.pass_case(n, a, b, first)
        assert tg.size == n and qs.shape[0] == 17
        r = am.rows_of(ids, tg)
        fin = np.isfinite(x).all(axis=1)
        good = x[fin]
        assert fi.top_separated(good, qs).all() and not fi.predicted_redo(good, qs).any() and fi.predicted_redo(x[~fin], qs).all()
        bad_at = np.flatnonzero((r >= 0) & ~fin[np.maximum(r, 0)])
        assert (bad_at < first).sum() == a and (bad_at >= first).sum() == b
        assert ((r < 0) & (np.arange(n) < first)).any() and ((r < 0) & (np.arange(n) >= first)).any()


def test_kmeans_inputs():
    import cluster_model as cm
    x, ids, tokens, kc, draws = fi.three_vector_tokens()
    v = cm.token_vectors(ids, x, tokens)
    assert len(np.unique(v, axis=0)) == 3
    c0 = np.stack([v[cm.pick(len(v), draws[i]) - 1] for i in range(kc)])
    assert fi.top_separated(v, c0).all() and fi.predicted_redo(v, c0).sum() > 0
    flags = fi.rounds_flagged(*fi.nan_tokens(fi.NAN_SEED))
    assert len(flags) == 10 and any(flags) and not all(flags) and not flags[0], flags


def test_encode_cases():
    """Part G: per case and position, the separation (distances equal to the prefix minimum or 8 brackets above it), the predicted
    redo set -- the ENC_NEAR items of the planted position or nothing --, finite values of ordinary magnitude (no scale condition),
    and the winner: the lowest index of the nearest copies."""
    S = fi.ENC_D // fi.ENC_M
    cases = fi.encode_cases()
    assert set(cases) >= {"16_in_tile0", "17_in_tile0", "16_in_last_tile", "17_in_last_tile", "compaction_12_then_10", "33_in_one_tile"}
    for name, (x, cb, winner, redone) in cases.items():
        assert x.shape == (70, fi.ENC_D) and cb.shape == (fi.ENC_M, fi.ENC_K, S), name
        assert np.isfinite(x).all() and np.isfinite(cb).all() and 1e-3 < np.abs(x).max() < 100 and 1e-3 < np.abs(cb).max() < 100
        for p in range(fi.ENC_M):
            xs = x[:, p * S:(p + 1) * S]
            assert fi.enc_separated(xs, cb[p]).all(), (name, p)
            pred = fi.enc_predicted_redo(xs, cb[p])
            want = np.zeros(70, bool)
            if p == fi.ENC_POS and redone:
                want[list(fi.ENC_NEAR)] = True
            assert np.array_equal(pred, want), (name, p)
        D, eps = fi.enc_dists(x[list(fi.ENC_NEAR), fi.ENC_POS * S:(fi.ENC_POS + 1) * S], cb[fi.ENC_POS])
        assert (np.argmin(D, axis=1) == winner).all() and (eps < 0.02).all(), name
    x, cb, _, _ = cases["compaction_12_then_10"]
    D, eps = fi.enc_dists(x[list(fi.ENC_NEAR), 2 * S:3 * S], cb[2])
    assert (D[:, 3] >= D[:, 140] + 8 * eps).all() and (D[:, 3:15] == D[:, 3:4]).all() and (D[:, :128].argmin(axis=1) == 3).all()
