"""CPU check of tests/join_bigk_inputs.py: the conditions under which tests/test_gpu_join_bigk.py is not vacuous.  The oracle
alone; nothing here needs a device.

The kNN-join's lists of more than 512 entries are written in closed form from a query's 2k smallest (distance, row) keys
(csrc/bigk.h) instead of by the guarded insertion.  Where no two rows of a query are equally far, any correct selection gives the
oracle's list; the closed form's tie rule is only tested by a query whose k-th place is tied, and decides ids (not just order)
only where the list at k is not a prefix of the list at k + 8."""
import numpy as np
import pytest

import join_bigk_inputs as jb


def test_table_repeats_every_row_four_times():
    t = jb.tables()
    for name in ("codes", "vectors", "coarse_id"):
        a = np.asarray(t[name])
        assert a.shape[0] == jb.N and all(np.array_equal(a[:jb.PERIOD], a[i * jb.PERIOD:(i + 1) * jb.PERIOD]) for i in range(1, 4)), name
    assert (np.diff(t["ids"]) > 0).all()
    tg = jb.all_targets()
    assert tg.size == 15000 and np.unique(tg).size == 15000 and tg.min() >= 1 and tg.max() <= jb.N
    odd = jb.odd_targets()
    assert np.unique(odd).size < odd.size and (odd > jb.N).sum() == 1
    qs, mask = jb.poisoned_queries()
    assert np.isnan(qs[2]).sum() == 1 and np.isinf(qs[5]).sum() == 1 and mask.sum() == 2 and np.isfinite(qs[~mask]).all()


def test_every_case_ties_across_the_kth_place(oracle):
    """In the list asked at k + 8, dist[k - 1] == dist[k] for at least one query of every (method, k) -- over the whole target
    array for every k; the cases with fewer targets add rounds and short lists -- and for some cases the list at k is not the first
    k entries of the list at k + 8: the tie rule decides ids."""
    ot = jb.oracle_table(oracle)
    rounds, short, decides, ties = [], [], 0, {}
    for method in jb.METHODS:
        for (k, alpha, nt, conf) in jb.CASES:
            exp, it = jb.expected(oracle, method, k, alpha, nt, conf)
            more, _ = oracle.ivpq_search_in(ot, jb.queries(), k + 8, jb.targets(nt), alpha, jb.PVF, method, use_target_lists=True,
                                            confidence=conf)
            filled = (more["id"] >= 0).sum(1)
            tied = [q for q in range(jb.Q) if filled[q] > k and more["dist"][q, k - 1] == more["dist"][q, k]]
            ties[(method, k)] = ties.get((method, k), 0) + len(tied)
            decides += sum(not np.array_equal(exp["id"][q], more["id"][q, :k]) for q in tied)
            rounds.append(it)
            short.append(int(((exp["id"] >= 0).sum(1) < k).sum()))
            print(f"method {method} k {k} alpha {alpha} targets {nt} conf {conf}: rounds {it}, tied queries {len(tied)}, short lists {short[-1]}")
    assert all(ties[(method, c[0])] > 0 for method in jb.METHODS for c in jb.CASES), ties
    assert max(rounds) > 1, rounds
    assert max(short) > 0, short
    assert decides > 0, "no case in which the tie rule decides ids"


@pytest.mark.parametrize("method", jb.METHODS)
def test_fewer_targets_than_k_fill_the_rest_with_the_sentinel(oracle, method):
    exp, _ = jb.expected(oracle, method, 2000, 1, 1500, 0.2)
    assert ((exp["id"] >= 0).sum(1) == 1500).all()
    assert (exp["id"][:, 1500:] == -1).all() and (exp["dist"][:, 1500:] == np.float32(1000.0)).all()


@pytest.mark.parametrize("method", jb.METHODS)
def test_poisoned_queries_leave_their_neighbours_alone(oracle, method):
    """The case of the GPU test's non-finite check: the poisoned queries accept no row, and the oracle answers the healthy ones as
    it does without them."""
    k, alpha, conf = jb.NONFINITE_CASE
    qs, mask = jb.poisoned_queries()
    bad, _ = oracle.ivpq_search_in(jb.oracle_table(oracle), qs, k, jb.targets(), alpha, jb.PVF, method, confidence=conf)
    exp, _ = jb.expected(oracle, method, k, alpha, None, conf)
    assert (bad["id"][mask] == -1).all()
    assert np.array_equal(bad["id"][~mask], exp["id"][~mask])
    assert np.array_equal(bad["dist"][~mask].view(np.uint32), exp["dist"][~mask].view(np.uint32))
