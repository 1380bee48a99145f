"""Inputs of the kNN-join by row id (include/freddy_gpu.h: freddy_gpu_knn_join_ids) and of the batched analogy over the kNN-join
(freddy_gpu_ivpq_analogy), shared by tests/test_join_ids_inputs_cpu.py (which proves with the oracle alone that they are what they claim
to be) and the GPU tests that run them.  Inputs only: nothing here touches a device.

Join: three ivpq tables of 8000 rows (ids 1 .. 8000) whose half vectors take the three ways sub_dist_rows_kernel loads a row --
  (50, 5, 64, 8)     half = 25: scalar loads, rows at offsets that are no multiple of 4 floats
  (64, 8, 16, 4)     half = 32: 16-byte loads
  (300, 12, 256, 16) half = 150: scalar loads, every row 16-byte aligned
-- 40 query rows, 3000 targets, and cases of which every shape runs one for more than one round.
Vector tables: the ivpq table's own rows; `more` = those and 100 rows the ivpq table does not hold (ids 9001 ..); `fewer` = every
third row (ids 3 r + 1: not serial), so most ids of the ivpq table have no row there."""
import functools

import numpy as np
import torch

import approx_analogy_model as am
import pv_model as pm
import util
from freddy_amd import index_build as ib

TABLE_ORDER, POSITIONAL = 0, 1
N, NQ = 8000, 40
SHAPES = ((50, 5, 64, 8), (64, 8, 16, 4), (300, 12, 256, 16))      # (d, m, K, k_coarse)
METHODS = (0, 1, 2)
CASES = ((5, 3, 20, 3000, 0.8), (5, 1, 3, 300, 0.3), (20, 1, 3, 300, 0.05), (60, 5, 20, 3000, 0.8))   # (k, alpha, pvf, T, confidence)
SUB_BATCH = (0, 3, 3, 17, 39)     # positions of the whole batch: the independence check, and what a positional call compacts to
FILLER = np.float32(1000.0)


def tables(shape):
    return util.shape_ivpq_tables(*shape, N)


def pin_args(t):
    return (t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])


def query_rows():
    return np.sort(np.random.default_rng(21).choice(N, NQ, replace=False))


def query_ids():
    return (query_rows() + 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def all_targets():
    t = np.random.default_rng(5).choice(np.arange(1, N + 1), 3000, replace=False).astype(np.int32)
    t.setflags(write=False)
    return t


def targets(T):
    return all_targets()[:T].copy()


@functools.lru_cache(maxsize=None)
def vec_table(shape, which):
    """-> (ids, x) of a vector table over the shape's corpus: "same", "more" or "fewer" """
    x = np.asarray(tables(shape)["vectors"], np.float32)
    if which == "same":
        ids, rows = np.arange(1, N + 1, dtype=np.int32), x
    elif which == "more":
        extra = -x[5::80][:100]
        ids, rows = np.concatenate([np.arange(1, N + 1), np.arange(9001, 9101)]).astype(np.int32), np.concatenate([x, extra])
    elif which == "fewer":
        ids, rows = (3 * np.arange(N // 3, dtype=np.int64) + 1).astype(np.int32), x[::3][:N // 3]
    else:
        raise ValueError(which)
    rows = np.ascontiguousarray(rows, np.float32)
    rows.setflags(write=False)
    return ids, rows


def model(ids, query_ids, rule):
    """The id rule in numpy: (sel, rows) -- the selected ids and the table row of each (-1: none)."""
    query_ids = np.asarray(query_ids, np.int32)
    row = {int(v): r for r, v in enumerate(ids)}
    if rule == TABLE_ORDER:
        sel = np.array(sorted({int(q) for q in query_ids if int(q) in row}), np.int32)
    else:
        sel = query_ids.copy()
    return sel, np.array([row.get(int(q), -1) for q in sel], np.int64)


def noisy_positional(ids):
    """the ids at SUB_BATCH's positions with unknown ids (one negative, one beyond the table, one in no table at all) around and
    between them: a repeated id is in SUB_BATCH already"""
    known = ids[list(SUB_BATCH)]
    return np.array([-7, known[0], known[1], 2 ** 30, known[2], known[3], 0, known[4], 10 ** 8], np.int32)


_expected = {}


def oracle_table(oracle, shape):
    key = ("table", shape)
    if key not in _expected:
        _expected[key] = oracle.ivpq_table(*pin_args(tables(shape)))
    return _expected[key]


def expected(oracle, shape, method, case, use_tl=True, rows=None):
    """The oracle's (lists, iterations) of ONE join over the vectors of `rows` (default: the 40 query rows) of the shape's table;
    computed once per session and shared."""
    k, alpha, pvf, T, conf = case
    key = (shape, method, case, use_tl, None if rows is None else tuple(int(r) for r in rows))
    if key not in _expected:
        x = np.asarray(tables(shape)["vectors"], np.float32)
        qs = x[query_rows() if rows is None else np.asarray(rows)]
        _expected[key] = oracle.ivpq_search_in(oracle_table(oracle, shape), qs, k, targets(T), alpha, pvf, method, use_target_lists=use_tl, confidence=conf)
    return _expected[key]


# ---- the analogy over the kNN-join: pv_model's table (20 000 x 300, ids 1 .. N) behind an ivpq index, approx_analogy_model's triples ----
AN_SHAPES = ((1, 4), (3, 23))     # (k, n_cand)


@functools.lru_cache(maxsize=None)
def analogy_tables():
    """-> (x, ids, the ivpq table's arrays)"""
    x, ids = pm.main_tables()[:2]
    t = ib.build_ivpq_index(torch.from_numpy(x), m=30, K=32, k_coarse=8, train_size=5000, iters=4, seed=7)
    return x, ids, t


@functools.lru_cache(maxsize=None)
def analogy_base():
    """3997 ids that are an input of no even-numbered triple, and three ids without a row, shuffled"""
    _, ids, _ = analogy_tables()
    t = am.main_triples()
    rng = np.random.default_rng(3)
    pool = ids[~np.isin(ids, t[::2].reshape(-1))]
    base = rng.permutation(np.concatenate([rng.choice(pool, 3997, replace=False), [-5, 0, 10 ** 8]])).astype(np.int32)
    base.setflags(write=False)
    return base


def analogy_target_sets():
    """name -> (targets, (alpha, pvf, confidence)); n_cand and the method come from the test"""
    _, ids, _ = analogy_tables()
    base, t7 = analogy_base(), am.main_triples()[7]
    return {
        "all": (ids.copy(), (3, 20, 0.8)),
        "base300": (base[:300].copy(), (1, 3, 0.3)),
        "base3": (base[:3].copy(), (1, 3, 0.3)),
        "inputs7": (t7.copy(), (1, 3, 0.3)),
        "inputs7+2": (np.concatenate([t7, base[:2]]).astype(np.int32), (1, 3, 0.3)),
    }
