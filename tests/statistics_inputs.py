"""Inputs of the statistics swap in tests/test_gpu_statistics.py, and of tests/test_statistics_inputs_cpu.py, which proves with
the oracle alone that the swap bites.

The table is util.ivpq_tables(N = 20 000) (64 cells).  Row A is the whole-table row (stat_google_vecs_norm_word).  Row B is
the model's row (tests/statistics_model.py) for a target column concentrated in a few cells: every row of the four largest
cells, every second of them a second time, 300 rows from anywhere and two ids no row has.  The join is asked for the column's
own tokens -- "joining against the tokens of another column with that column's statistics".  With A the traversal believes the
targets spread like the table and stops after a cell or two; with B it knows where they are and takes up to 41 cells, so the
rows give different cell counts, different iteration counts and different lists (SEED and CONFIDENCE were picked so that this
holds; the CPU test keeps it true)."""
import functools

import numpy as np

import statistics_model as sm
import util

N, Q = 20000, 16
SEED = 2
CONFIDENCE = 0.8
CALLS = [(5, 3), (10, 10)]   # (k, alpha)
PVF = 20
METHODS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def tables():
    return util.ivpq_tables(N=N)


def cells():
    return tables()["coarse"].shape[1] ** 2


@functools.lru_cache(maxsize=None)
def column():
    """the target column's row ids, with multiplicity and two unknown ids"""
    t = tables()
    rng = np.random.default_rng(SEED)
    big = np.argsort(-np.bincount(t["coarse_id"], minlength=cells()), kind="stable")[:4]
    rows = np.nonzero(np.isin(t["coarse_id"], big))[0]
    other = rng.choice(N, 300, replace=False)
    return np.concatenate([t["ids"][rows], t["ids"][rows[::2]], t["ids"][other], [N + 50, -3]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def targets():
    """the column's distinct tokens that have a row: what the join is asked for"""
    col = column()
    return np.unique(col[(col >= 1) & (col <= N)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def queries():
    return util.queries_from_corpus(N, Q, seed=40 + SEED)[1]


@functools.lru_cache(maxsize=None)
def row_a():
    t = tables()
    return sm.create_statistics(t["ids"], t["coarse_id"], cells())[0]


@functools.lru_cache(maxsize=None)
def row_b():
    t = tables()
    return sm.create_statistics(t["ids"], t["coarse_id"], cells(), column())[0]


def pin_args(stats):
    t = tables()
    return (t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], stats)


_expected = {}


def oracle_table(oracle, which):
    if which not in _expected:
        _expected[which] = oracle.ivpq_table(*pin_args(row_a() if which == "A" else row_b()))
    return _expected[which]


def expected(oracle, which, method, k, alpha, use_tl=True):
    """The oracle's (lists, iterations) of a call over the table with row `which` ("A" / "B"); computed once and shared."""
    key = (which, method, k, alpha, use_tl)
    if key not in _expected:
        _expected[key] = oracle.ivpq_search_in(oracle_table(oracle, which), queries(), k, targets(), alpha, PVF, method,
                                               use_target_lists=use_tl, confidence=CONFIDENCE)
    return _expected[key]
