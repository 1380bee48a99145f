"""Inputs of tests/test_gpu_join_bigk.py (the kNN-join with methods 0 / 1 and 512 < k <= 4096), and of
tests/test_join_bigk_inputs_cpu.py, which proves with the oracle alone that they exercise what the GPU test is about.

The table is util.ivpq_tables(N = 20 000) with the codes, vectors and cells of rows 0 .. 4999 repeated four times: every
distance, ADC and exact alike, occurs four times per query, so the k-th place of a list is tied for most queries and the rule
"equal distances end in descending arrival; a tie at the k-th distance is accepted iff fewer than k rows at or below it
arrived before" decides which IDS a list holds, not only their order."""
import functools

import numpy as np

import util

N, PERIOD, Q = 20000, 5000, 8
METHODS = (0, 1)
# (k, alpha, number of targets or None for all, confidence)
CASES = [(513, 3, None, 0.8), (600, 1, None, 0.8), (2000, 2, None, 0.8), (4096, 1, None, 0.8), (600, 1, 700, 0.3),
         (2000, 1, 1500, 0.2)]
PVF = 4   # (methods 0 / 1 do not read it)
NONFINITE_CASE = (600, 3, 0.8)   # (k, alpha, confidence) of the non-finite check, all targets


@functools.lru_cache(maxsize=None)
def tables():
    t = dict(util.ivpq_tables(N=N))
    rep = np.arange(N) % PERIOD
    for name in ("codes", "vectors", "coarse_id"):
        t[name] = np.ascontiguousarray(np.asarray(t[name])[rep])
    return t


def pin_args(t=None):
    t = t or tables()
    return (t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])


@functools.lru_cache(maxsize=None)
def queries():
    return util.queries_from_corpus(N, Q, seed=29)[1]


@functools.lru_cache(maxsize=None)
def all_targets():
    return np.random.default_rng(12).choice(np.arange(1, N + 1), size=15000, replace=False).astype(np.int32)


def targets(n=None):
    t = all_targets()
    return t if n is None else t[:n].copy()


def odd_targets():
    """duplicates and an unknown id among 3000 targets"""
    t = all_targets()
    return np.concatenate([t[:3000], t[:40], np.array([N + 100], np.int32), t[100:130]]).astype(np.int32)


def poisoned_queries():
    """-> (queries with a NaN in query 2 and an Inf in query 5, mask of the poisoned ones)"""
    qs = queries().copy()
    qs[2, 7] = np.nan
    qs[5, 291] = np.inf
    mask = np.zeros(Q, bool)
    mask[[2, 5]] = True
    return qs, mask


_expected = {}


def expected(oracle, method, k, alpha, n_targets, confidence, use_tl=True, double_threshold=10000000):
    """The oracle's (lists, iterations) of a case; computed once per session and shared."""
    key = (method, k, alpha, n_targets, confidence, use_tl, double_threshold)
    if key not in _expected:
        if "ot" not in _expected:
            _expected["ot"] = oracle.ivpq_table(*pin_args())
        _expected[key] = oracle.ivpq_search_in(_expected["ot"], queries(), k, targets(n_targets), alpha, PVF, method,
                                               use_target_lists=use_tl, confidence=confidence, double_threshold=double_threshold)
    return _expected[key]


def oracle_table(oracle):
    if "ot" not in _expected:
        _expected["ot"] = oracle.ivpq_table(*pin_args())
    return _expected["ot"]
