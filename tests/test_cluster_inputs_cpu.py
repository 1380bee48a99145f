"""The numpy model of freddy_gpu_cluster (tests/cluster_model.py) and the steered cases of tests/test_gpu_cluster.py
(tests/cluster_inputs.py), proven without a device: the model agrees with the existing restatement of generic_cluster, and the traces
of the cases reach between them every situation the GPU test is there for."""
import numpy as np
import pytest

import assign_model as am
import cluster_inputs as ci
import cluster_model as cm


@pytest.mark.parametrize("method", ["exact", "pq"])
def test_model_equals_the_existing_restatement(oracle, method):
    """rounds = 10: the clusters of the model equal _cluster_reference (tests/test_gpu_udf.py) fed with the assign model's rows."""
    from test_gpu_udf import _cluster_reference
    x, ids, cb, codes = ci.tables("25d_m5")
    rng = np.random.default_rng(7)
    n, kc = 90, 5
    tokens = np.sort(rng.choice(ids, n, replace=False)).astype(np.int32)
    draws = rng.random(cm.n_draws(kc, 10))

    def rows(cent):
        if method == "exact":
            q, s = am.exact_assign(ids, x, cent, tokens)
        else:
            q, s = am.pq_assign(oracle, cb, ids, codes, cent, tokens, sentinel=1000.0)
        return [(s[i], int(q[i]) + 1, i + 1) for i in range(n) if q[i] >= 0]

    exp = _cluster_reference(rows, x[tokens - 1], n, kc, draws)
    case = dict(shape="25d_m5", method=method, tokens=tokens, kc=kc, rounds=10, draws=draws, sentinel=1000.0)
    got = ci.run_model(case, oracle)
    assert np.array_equal(got["clusters"], exp)
    assert set(np.unique(got["clusters"])) <= set(range(1, kc + 1))


def test_pick_of_the_model():
    assert cm.pick(10, 0.0) == 1 and cm.pick(10, 1.0 - 2.0 ** -53) == 10 and cm.pick(1, 0.7) == 1
    assert cm.pick(4, 0.25) == 2 and cm.pick(4, 0.5) == 2 and cm.pick(4, 0.75) == 4      # 1.5 -> 2, 2.5 -> 2, 3.5 -> 4: half to even
    assert cm.pick(2 ** 31 - 1, 1.0 - 2.0 ** -53) == 2 ** 31 - 1 and cm.pick(7, -3.0) == 1 and cm.pick(7, 9.0) == 7


def test_the_cases_reach_what_they_are_there_for(oracle):
    reached = {}
    for case in ci.steered_cases():
        out = ci.run_model(case, oracle)
        reached[case["name"]] = ci.reached(case, out)
        # the draws are all there and every sampled position is a member's
        assert case["draws"].size == cm.n_draws(case["kc"], case["rounds"])
        for J, i, t, x, ln, pos in out["trace"]:
            assert t < 0 or (1 <= x <= ln and pos >= 0)            # (a rank never lies beyond the members: |members| >= lens)
    union = set().union(*reached.values())
    assert union >= ci.WANTED, (ci.WANTED - union, reached)
    # each case is there for something of its own
    assert {"wave_edge", "chunk_edge", "drawn_twice", "empty_before_sampling", "rank_1", "rank_len"} <= reached["ranks"]
    assert "step_edge" in reached["step"]
    assert {"stale_member", "cluster_0"} <= reached["unclaimed"]
    assert "kc_above_n" in reached["kc_above_n"] and "kc_1" in reached["kc_1"]
