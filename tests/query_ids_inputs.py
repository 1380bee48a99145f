"""Inputs of the searches by row id (include/freddy_gpu.h: freddy_gpu_*_search_ids), shared by tests/test_query_ids_inputs_cpu.py
(which proves on the CPU that they are what they claim to be) and tests/test_gpu_query_ids.py (which runs them).  Inputs and a numpy
model of the id rule only: nothing here touches a device.

A case is an ANN table (ivf, and for the 300-d / K = 256 shape pq) over the rows of a corpus with ids 1 .. N, and a VECTOR table
(ids, x) that is a different table on purpose: NV = 4999 rows (no multiple of 64) with the ids 3 r + 1 -- not serial, so a shortcut
for serial ids cannot hide a wrong row lookup -- whose first rows are corpus rows and whose last 999 are negated corpus rows, vectors
the ANN table does not hold.  The ANN table in turn holds ids (2, 3, 5, ...) the vector table lacks."""
import functools

import numpy as np
import torch

import dev_contract_inputs as dci
import pv_model as pm
import util
from freddy_amd import index_build as ib

TABLE_ORDER, POSITIONAL = 0, 1
NV = 4999
COUNTS = (1, 2, 8, 9, 64, 65)     # both sides of the in-place bound of a host-buffer call (8) and of a wave (64)
SHAPES = ("d300_k256", "d300_k1024", "d25", "d8")
STRAGGLER_KEY = ("300", 256, 5, False)   # the thinned table of dev_contract_inputs


def vec_ids(n):
    return (3 * np.arange(n, dtype=np.int64) + 1).astype(np.int32)


def _vec_table(x):
    """NV rows: 4000 corpus rows spread over the corpus, then 999 negated ones"""
    rows = np.ascontiguousarray(np.concatenate([x[::x.shape[0] // 4000][:NV - 999], -x[7::5][:999]]).astype(np.float32))
    assert rows.shape[0] == NV
    rows.setflags(write=False)
    return vec_ids(NV), rows


@functools.lru_cache(maxsize=None)
def case(shape):
    """-> dict: ivf (the table's arrays), pq (d300_k256 only), vec_ids, vec_x, W"""
    if shape == "d300_k256":      # 75 sixteen-byte units per row; the one-byte slab scan
        x, _, _, ivf, pq = pm.main_tables()
        out = {"ivf": ivf, "pq": pq, "W": 4}
    elif shape == "d300_k1024":   # the int16 slab scan; a tiny k-means
        x = util.corpus(20000).numpy()[:6000]
        out = {"ivf": ib.build_ivf_index(torch.from_numpy(x), C=16, m=12, K=1024, train_size=2000, iters=2, seed=3), "W": 4}
    elif shape == "d25":          # the reference's shipped shape: the scalar gather, the multi.h scan
        x = util.shape_corpus(8000, 25).numpy()
        out = {"ivf": ib.build_ivf_index(torch.from_numpy(x), C=16, m=5, K=64, train_size=4000, iters=3, seed=3), "W": 4}
    elif shape == "d8":           # a row of two sixteen-byte units: shorter than a wave's worth
        x = util.shape_corpus(8000, 8).numpy()
        out = {"ivf": ib.build_ivf_index(torch.from_numpy(x), C=16, m=2, K=32, train_size=4000, iters=3, seed=3), "W": 4}
    else:
        raise ValueError(shape)
    out["vec_ids"], out["vec_x"] = _vec_table(x)
    return out


def ivf_args(t):
    return t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"]


def known_ids(ids, n, seed):
    """n distinct ids of the table in a seeded order that is not ascending; from n = 2 on the ids of row 0 and of the last row are among them"""
    rng = np.random.default_rng(seed)
    inner = rng.choice(np.arange(1, ids.size - 1), size=max(n - 2, 0), replace=False)
    rows = np.concatenate([[ids.size - 1, 0][:min(n, 2)], inner]) if n >= 2 else rng.choice(ids.size, size=1)
    out = ids[rows[:n].astype(np.int64)]
    if n >= 3:
        out = out[rng.permutation(n)]
    return out.astype(np.int32)


def noisy_ids(ids, known, seed):
    """`known` with a quarter of it repeated and with ids that have no row -- below the smallest id, above the largest, inside a gap --
    in the first, a middle and the last slot and spread over the rest"""
    rng = np.random.default_rng(1000 + seed)
    gaps = ids[rng.choice(ids.size - 1, size=3)] + 1                    # (3 r + 2: between two ids)
    unknown = np.concatenate([[ids[0] - 1, -7, ids[-1] + 1, 2 ** 30], gaps]).astype(np.int32)
    dup = known[rng.choice(known.size, size=max(1, known.size // 4))]
    mid = rng.permutation(np.concatenate([known, dup, unknown[3:]]))
    half = mid.size // 2
    return np.concatenate([[unknown[0]], mid[:half], [unknown[1]], mid[half:], [unknown[2]]]).astype(np.int32)


def model(ids, query_ids, rule):
    """The id rule in numpy: (sel, rows) -- the selected ids and the table row of each (-1: none)."""
    query_ids = np.asarray(query_ids, np.int32)
    row = {int(v): r for r, v in enumerate(ids)}
    if rule == TABLE_ORDER:
        sel = np.array(sorted({int(q) for q in query_ids if int(q) in row}), np.int32)
    else:
        sel = query_ids.copy()
    return sel, np.array([row.get(int(q), -1) for q in sel], np.int64)


# ---- stragglers: the thinned table of dev_contract_inputs, its "mixed" batch (designed unfinished queries among finished corpus rows)
# as the vector table ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straggler_case(W):
    c = dci.case(*STRAGGLER_KEY)
    qs, names = dci.batches(*STRAGGLER_KEY, W)["mixed"]
    return {"c": c, "vec_ids": vec_ids(qs.shape[0]), "vec_x": qs, "names": names}


def straggler_runs():
    """(W, found rule, sentinel) the tests run: both rules of the plain search at four probes, and the batch UDF's (W = 1, 100.0)"""
    c = dci.case(*STRAGGLER_KEY)
    return [(4, 0, c["sentinel"]), (4, 1, c["sentinel"]), (1, 2, 100.0)]
