"""What post verification (pv.h, freddy_gpu_ivfadc_search_pv / freddy_gpu_pq_search_pv) must return, from the oracle alone:
  1. the approximate search at k * pvf (Oracle.ivfadc_search_many / pq_search / pq_search_in),
  2. its ids < 0 and its ids without a vector dropped,
  3. Oracle.exact_knn over exactly those candidates.
Also the shared tables of the GPU tests (built once per process) and a literal restatement of the host mirror's knn_pv loop."""
import functools

import numpy as np
import torch

import util
from freddy_amd import index_build as ib

ENTRY = np.dtype([("id", np.int32), ("dist", np.float32)])


def candidates(list_ids, vec_ids):
    """step 2 for one query: (ids >= 0 of the list, those of them that have a vector)"""
    ids = np.asarray(list_ids, np.int32)
    ids = ids[ids >= 0]
    return ids, ids[np.isin(ids, vec_ids)]


def rerank(oracle, x, vec_ids, q, k, cand):
    """step 3 (an empty candidate set is an empty list, never the whole table)"""
    if cand.size == 0:
        return np.empty(0, ENTRY)
    return oracle.exact_knn(x, vec_ids, q, k, cand)


def expected(oracle, lists, x, vec_ids, qs, k):
    """lists: [Q][k * pvf] ids of step 1 -> (list of per-query entries, candidates per query, scored per query)"""
    out, n_cand, n_scored = [], [], []
    for q, l in zip(qs, lists):
        ids, have = candidates(l, vec_ids)
        n_cand.append(ids.size)
        n_scored.append(have.size)
        out.append(rerank(oracle, x, vec_ids, q, k, have))
    return out, np.array(n_cand, np.int64), np.array(n_scored, np.int64)


def ivf_lists(oracle, table, qs, kc, W, sentinel=1000.0, found_rule=0):
    return oracle.ivfadc_search_many(table, qs, kc, W, sentinel=sentinel, found_rule=found_rule, n_threads=8)["id"]


def pq_lists(oracle, table, qs, kc, subset_ids=None):
    if subset_ids is None:
        return np.stack([oracle.pq_search(table, q, kc)["id"] for q in qs])
    return np.stack([oracle.pq_search_in(table, q, kc, subset_ids)["id"] for q in qs])


def same(gi, gs, exp, k, what):
    """ids and similarity bits of every query equal the model's; (-1, -inf) beyond its rows"""
    assert gi.shape == (len(exp), k) and gs.shape == (len(exp), k), what
    for qi, e in enumerate(exp):
        n = len(e)
        assert gi[qi, :n].tolist() == e["id"].tolist(), (what, qi)
        assert np.array_equal(gs[qi, :n].view(np.uint32), e["dist"].view(np.uint32)), (what, qi)
        assert (gi[qi, n:] == -1).all() and np.isneginf(gs[qi, n:]).all(), (what, qi)


def knn_pv_loop(x, vec_ids, q, k, list_ids):
    """host/freddy_udf.cpp knn_pv, literally: skip ids < 0, skip ids without a vector, the binary32 chain scalar += v1[i] * v2[i],
    sort by (similarity DESC, id ASC), first k."""
    cand = []
    for i in list_ids:
        if i < 0:
            continue
        r = int(np.searchsorted(vec_ids, i))
        if r >= vec_ids.size or vec_ids[r] != i:
            continue
        s = np.float32(0.0)
        for a, b in zip(q, x[r]):
            s = np.float32(s + np.float32(a * b))
        cand.append((int(i), s))
    cand.sort(key=lambda c: (-float(c[1]), c[0]))
    return cand[:k]


# ---- the main case's tables: 20 000 x 300, C = 32, m = 12, K = 256, 40 exact duplicate rows --------------------------------------
@functools.lru_cache(maxsize=None)
def main_tables():
    N = 20000
    x = util.corpus(N).numpy().copy()
    x[N // 2:N // 2 + 40] = x[100:140]              # duplicate rows: equal similarities, the id order decides
    xt = torch.from_numpy(x)
    ivf = ib.build_ivf_index(xt, C=32, m=12, K=256, train_size=5000, iters=4, seed=5)
    pq = ib.build_pq_index(xt, m=12, K=256, train_size=5000, iters=4, seed=6)
    ids = np.arange(1, N + 1, dtype=np.int32)       # (make_corpus: ids 1..N in row order)
    qs = x[::100][:200].copy()
    qs[3] = -qs[3]                                  # negative similarities
    qs[6] = x[100]                                  # an exact copy of a table row -- of one that has a duplicate
    qs[10:20] = x[N // 2 + 5:N // 2 + 15]
    return x, ids, qs, ivf, pq
