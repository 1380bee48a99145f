"""Inputs with a KNOWN set of unfinished queries for the device-pointer searches' status word (include/freddy_gpu.h:
freddy_gpu_ivfadc_search_dev), shared by tests/test_dev_contract_inputs_cpu.py (which proves on the CPU that they are what they
claim to be) and tests/test_gpu_dev_contract.py (which runs them).  Inputs and the oracle's lists only: nothing here touches a device.

Definitions (oracle/freddy_oracle.h): a query is UNFINISHED iff found < k after the first probing round; its ROUND-ONE LIST is the
oracle's list with max_rounds = 1.

The tables: util.ivf_tables(N, C = 64, K) for 300-d / m = 12 (N = 20 000; 60 000 where k = 600 needs cells of 600 rows) and
util.shape_ivf_tables(64, 8, 16, 16, 8000) for the multi-scan path, with nine cells thinned by dropping rows (list_off rebuilt):
  E  an empty cell                                  O  a cell of one row
  M  a cell of k - 1 rows                           X  a cell of exactly k rows
  S  a cell of exactly k rows, the k - 1 nearest its centroid and the farthest one; the case's sentinel IS the farthest
     row's distance from the centroid, so "dist < sentinel" (freddy.c:128-131) rejects that row: the centroid's query is finished
     under the rows rule (k rows retrieved) and unfinished under the accepted rule (k - 1 insertions)
  G  a group of four cells, the four nearest of its first cell's centroid, of (k - 1) // 4 rows each: fewer than k together
The rows a thinned cell keeps are those nearest its centroid.  `ties`: every second row of every list gets its predecessor's
codes first, so every candidate set holds equal distances (merge_replay_kernel's replay path).

Queries: the centroids of E, O, M, X, S; the centroid of G's first cell and seven copies of it moved by a thousandth of its
length (the same four nearest cells); corpus rows.  With W = 1 the centroids of E, O, M and the eight of G are unfinished by
design, with W = 4 the eight of G; X is finished; S tells the rules apart at W = 1.  Which corpus rows are finished is read off
the oracle (the sentinel lies inside the data, so the accepted rule depends on the distances).  Three batches per (case, W):
  none   corpus rows and X that are finished under every rule the tests run        (Q = 150)
  all    designed queries that are unfinished under every such rule                 (Q = 8 .. 11)
  mixed  every designed query among corpus rows, in a seeded order                  (Q = 300)"""
import functools

import numpy as np

import util
from oracle.oracle import Oracle

f32 = np.float32
N_GROUP = 4
Q_NONE, Q_MIXED = 150, 300
RULES = {1: (0, 1, 2), 4: (0, 1)}   # W -> the found rules the tests run (FREDDY_FOUND_BATCH_UDF needs W == 1)
BATCHES = ("none", "mixed", "all")
# (shape, K, k, ties) -> the W the tests run: every table tests/test_gpu_dev_contract.py pins.  k = 600 with one probe has no
# finished query on these tables (cells of 600 rows are the exception), so it runs with four only.
CASES = {("300", 256, 5, False): (1, 4), ("300", 256, 32, False): (1, 4), ("300", 1024, 5, False): (1, 4), ("300", 1024, 32, False): (1, 4),
         ("300", 256, 5, True): (1, 4), ("300", 256, 40, False): (1, 4), ("300", 256, 600, False): (4,), ("64", 16, 5, False): (1, 4)}


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


def _base(shape, K, k):
    if shape == "300":
        N = 60000 if k > 300 else 20000
        return util.ivf_tables(N=N, C=64, K=K), util.corpus(N).numpy()
    assert shape == "64" and K == 16
    return util.shape_ivf_tables(64, 8, 16, 16, 8000), util.shape_corpus(8000, 64).numpy()


@functools.lru_cache(maxsize=None)
def case(shape="300", K=256, k=5, ties=False):
    """The thinned table of (shape, K, k): dict with the table's arrays (coarse, codebook, list_off, ids, codes), the oracle's
    handle `ot`, the cells E O M X S and G (a list), `sentinel`, the designed queries `designed` (name -> vector) and 800 corpus rows `corpus`."""
    o = oracle()
    t, x = _base(shape, K, k)
    coarse, cb = np.asarray(t["coarse"], f32), np.asarray(t["codebook"], f32)
    lo = np.asarray(t["list_off"]).astype(np.int64)
    ids, codes = np.array(t["ids"], np.int32), np.array(t["codes"], np.int16)
    C, d, m = coarse.shape[0], coarse.shape[1], cb.shape[0]
    if ties:
        for c in range(C):
            a, n2 = lo[c], (lo[c + 1] - lo[c]) // 2 * 2
            codes[a + 1:a + n2:2] = codes[a:a + n2:2]
    sizes = np.diff(lo)
    # a row's distance from its own cell's centroid: the LUT of the zero residual (float64 sums: for ranking the rows only)
    lut0 = o.lut(np.zeros(d, f32), cb)
    own = lut0.reshape(m, K)[np.arange(m)[None, :], codes].astype(np.float64).sum(1)
    by_size = np.argsort(sizes, kind="stable")
    X, S = int(by_size[-1]), int(by_size[-2])
    cd = ((coarse[:, None, :].astype(np.float64) - coarse[None].astype(np.float64)) ** 2).sum(-1)
    for A in by_size:
        G = [int(c) for c in np.argsort(cd[A], kind="stable")[:N_GROUP]]
        if not set(G) & {X, S}:
            break
    rest = [int(c) for c in by_size if c not in G and c not in (X, S)]
    E, O, M = rest[0], rest[1], rest[-1]
    assert sizes[X] >= k and sizes[S] >= k and sizes[M] >= k - 1 and G[0] == A
    keep = np.ones(ids.size, bool)
    far_row = None
    for c, n, far in [(E, 0, False), (O, 1, False), (M, k - 1, False), (X, k, False), (S, k, True)] + [(g, (k - 1) // N_GROUP, False) for g in G]:
        rows = np.arange(lo[c], lo[c + 1])
        near = rows[np.argsort(own[rows], kind="stable")]
        keep[rows] = False
        keep[near[:n - 1] if far else near[:n]] = True
        if far:
            far_row = int(near[-1])
            keep[far_row] = True
    # the reference's own arithmetic for that row and the query coarse[S].  (k = 600: hardly a corpus row has 600 rows nearer than
    # that, the accepted rule would leave no finished query; that case runs with four probes, where S decides nothing, and 1000.0)
    sentinel = float(o.adc(lut0, codes[far_row], K)) if k <= 64 else 1000.0
    cell_of = np.repeat(np.arange(C), sizes)
    new_off = np.concatenate([[0], np.cumsum(np.bincount(cell_of[keep], minlength=C))]).astype(np.int32)
    out = {"coarse": coarse, "codebook": cb, "list_off": new_off, "ids": ids[keep], "codes": codes[keep],
           "cells": {"E": E, "O": O, "M": M, "X": X, "S": S}, "G": G, "sentinel": sentinel, "k": k, "K": K}
    out["ot"] = o.ivf_table(coarse, cb, new_off, out["ids"], out["codes"])
    rng = np.random.default_rng(77 + k)
    designed = {name: coarse[c].copy() for name, c in out["cells"].items()}
    designed["G0"] = coarse[A].copy()
    step = 1e-3 * float(np.linalg.norm(coarse[A])) / np.sqrt(d)
    for j in range(1, 8):
        designed[f"G{j}"] = (coarse[A] + step * rng.standard_normal(d)).astype(f32)
    out["designed"] = designed
    out["corpus"] = x[np.sort(rng.choice(x.shape[0], size=800, replace=False))].astype(f32)
    for a in (out["list_off"], out["ids"], out["codes"], out["corpus"]):
        a.setflags(write=False)
    return out


def search(c, qs, k, W, rule, max_rounds, sentinel=None):
    """The oracle's (lists, found, rounds) on the case's table.  Rule 2 is ivfadc_batch_search itself (W = 1, sentinel 100.0)."""
    o = oracle()
    if rule == 2:
        assert W == 1
        return o.ivfadc_batch_search(c["ot"], qs, k, max_rounds=max_rounds)
    return o.ivfadc_search_many(c["ot"], qs, k, W, sentinel=c["sentinel"] if sentinel is None else sentinel, found_rule=rule,
                                max_rounds=max_rounds)


def sentinel_of(c, rule):
    return 100.0 if rule == 2 else c["sentinel"]


@functools.lru_cache(maxsize=None)
def batches(shape, K, k, ties, W):
    """{"none" | "mixed" | "all": (queries [Q][d], names [Q])}; a corpus row's name is ""."""
    c = case(shape, K, k, ties)
    names = list(c["designed"]) + [""] * len(c["corpus"])
    qs = np.concatenate([np.stack(list(c["designed"].values())), c["corpus"]]).astype(f32)
    unfinished = np.stack([search(c, qs, k, W, rule, 1)[1] < k for rule in RULES[W]])
    never, always = unfinished.all(0), ~unfinished.any(0)
    n_designed = len(c["designed"])
    is_corpus = np.arange(len(names)) >= n_designed
    none = np.nonzero(always & (is_corpus | (np.array(names) == "X")))[0][:Q_NONE]
    every = np.nonzero(never & ~is_corpus)[0]
    fill = np.nonzero(always & is_corpus)[0][:Q_MIXED - n_designed]
    mixed = np.random.default_rng(5).permutation(np.concatenate([np.arange(n_designed), fill]))
    out = {}
    for name, rows in (("none", none), ("mixed", mixed), ("all", every)):
        q = qs[rows].copy()
        q.setflags(write=False)
        out[name] = (q, [names[r] for r in rows])
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, K, k, ties, W, rule, batch):
    """The oracle's account of one batch: round-one lists, which queries are unfinished, the uncapped lists."""
    c = case(shape, K, k, ties)
    qs, _ = batches(shape, K, k, ties, W)[batch]
    one, found, _ = search(c, qs, k, W, rule, 1)
    final, _, rounds = search(c, qs, k, W, rule, 0)
    return {"round_one": one, "unfinished": found < k, "final": final, "rounds": rounds}
