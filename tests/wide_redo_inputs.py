"""Inputs for the redo paths of exact kNN's two newer routes (tests/test_gpu_exact_redo_variants.py runs them,
tests/test_wide_redo_inputs_cpu.py proves them): lists of 33 .. 1024 rows (option exact_filter_k) over tests/redo_inputs.py's
table, and the wide filter (option exact_wide) over the same construction at d = 516.  Inputs only: nothing here touches a device.

Both tables: 20 000 rows, rows 5000 .. 14999 overwritten by row 4999 -- 10 001 equal rows, more than the 8 192 rows filter_plan_k
gives a candidate buffer there for every k <= 1024.  The HOT query is row 4999: the copies tie for the best similarity, the
threshold (the k-th largest of the sample, k <= 10 001) is their score, and all of them are candidates.  HEALTHY queries are rows
below 4999, drawn once in a fixed order and kept while -- in float64 -- their K-th best similarity exceeds the copies' by GAP and
at most half a buffer of rows comes within GAP of it, K the largest k the tests use on that table (the conditions only relax for
a smaller k).  redo_inputs.queries() itself does not qualify beyond k = 40: at k = 100 three, at k = 600 eight of its 70 queries
have the copies within 0.05 of their k-th best (the CPU test asserts that a replacement was needed)."""
import functools

import numpy as np

import redo_inputs as ri
import util

N, WIDE_D = ri.N, 516
ORIGINAL, COPY_ROWS, CAP, GAP, N_LIVE = ri.ORIGINAL, ri.COPY_ROWS, ri.CAP, ri.GAP, ri.N_LIVE
NARROW_KS, NARROW_K_MAX = (40, 100, 600), 600       # V = pick_V(k) = 1, 2 and 16
WIDE_KS, WIDE_K_MAX = (5, 32, 100), 100
HOT_AT = ((70, 0), (70, 40), (70, 63), (70, 64), (70, 69), (1, 0))     # (Q, position): tile 0, tile 1, the ends of the pass of 64, the pass of 6, a call of one
POISONS = ("nan", "pos_inf", "all_nan")             # util.QUERY_POISONS kinds


@functools.lru_cache(maxsize=None)
def wide_table():
    """(x[N][WIDE_D] float32, ids[N] int32), read-only: 41 MB"""
    x = util.shape_corpus(N, WIDE_D).numpy().copy()
    x[5000:15000] = x[ORIGINAL]
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    x.setflags(write=False)
    ids.setflags(write=False)
    return x, ids


def table(wide):
    return wide_table() if wide else ri.table()


@functools.lru_cache(maxsize=None)
def healthy_rows(wide):
    """N_LIVE rows below ORIGINAL in drawing order that satisfy the module's conditions at K = WIDE_K_MAX / NARROW_K_MAX"""
    x, _ = table(wide)
    K = WIDE_K_MAX if wide else NARROW_K_MAX
    x64 = x.astype(np.float64)
    drawn = np.random.default_rng(8 + int(wide)).choice(ORIGINAL, 400, replace=False)
    s = x64 @ x64[drawn].T                                   # [N][400]
    kth = -np.partition(-s, K - 1, axis=0)[K - 1]
    near = (s >= kth - GAP).sum(0)
    keep = drawn[(kth - s[ORIGINAL] >= GAP) & (near <= CAP // 2)][:N_LIVE]
    assert keep.size == N_LIVE
    keep.setflags(write=False)
    return keep


def hot_query(wide):
    return table(wide)[0][ORIGINAL].copy()


def bad_query(q, kind, seed=0):
    """util.poison_query: one NaN or +Inf in the first of twelve sub-vectors, or every element a NaN"""
    return util.poison_query(q, kind, 12, np.random.default_rng(seed))


def queries(wide, Q=N_LIVE, hot_at=(), bad=None):
    """[Q][d]: the healthy queries with the hot query (bad = None) or bad_query(healthy query, bad) at the positions hot_at"""
    qs = table(wide)[0][healthy_rows(wide)[:Q]].copy()
    for i in hot_at:
        qs[i] = hot_query(wide) if bad is None else bad_query(qs[i], bad, seed=i)
    return qs
