"""What the batched approximate analogies (approx_analogy.h; freddy_gpu_ivfadc_analogy / freddy_gpu_pq_analogy) must return, from the
oracle alone:
  1. raw = vec_plus(vec_minus(v3, v1), v2), unit = vec_normalize(raw)        (Oracle.vec_minus / vec_plus / vec_normalize),
  2. the approximate search for unit at n_cand                               (Oracle.ivfadc_search_many / pq_search / pq_search_in),
  3. its ids < 0, its ids without a vector and the three inputs dropped,
  4. Oracle.exact_knn(x, ids, RAW, k, the rest).
A triple with an id that has no vector is the SQL's empty join: no rows, not searched.  Also the triples of the GPU tests' main case
(with the properties they must have asserted on this model's data) and a literal restatement of analogy_common's host loop."""
import functools

import numpy as np

import pv_model as pm


def build_queries(oracle, x, vec_ids, triples):
    """step 1: (valid[Q], raw[Q'][d], unit[Q'][d]) -- Q' = the triples whose three ids have a vector, in order"""
    t = np.asarray(triples, np.int32).reshape(-1, 3)
    vec_ids = np.asarray(vec_ids, np.int32)
    rows = np.searchsorted(vec_ids, t)
    valid = ((rows < vec_ids.size) & (vec_ids[np.minimum(rows, vec_ids.size - 1)] == t)).all(axis=1)
    raw = np.empty((int(valid.sum()), x.shape[1]), np.float32)
    unit = np.empty_like(raw)
    with np.errstate(all="ignore"):
        for j, (r1, r2, r3) in enumerate(rows[valid]):
            raw[j] = oracle.vec_plus(oracle.vec_minus(x[r3], x[r1]), x[r2])
            unit[j] = oracle.vec_normalize(raw[j])
    return valid, raw, unit


def expected(oracle, lists, valid, raw, x, vec_ids, triples, k):
    """steps 3 and 4.  lists: [Q'][n_cand] ids of step 2 -> (per-triple entries, an empty list for an invalid triple; the stats)"""
    t = np.asarray(triples, np.int32).reshape(-1, 3)
    out, j, n_cand, n_scored = [], 0, 0, 0
    for q in range(t.shape[0]):
        if not valid[q]:
            out.append(np.empty(0, pm.ENTRY))
            continue
        ids, have = pm.candidates(lists[j], vec_ids)
        keep = have[~np.isin(have, t[q])]
        n_cand += ids.size
        n_scored += keep.size
        out.append(pm.rerank(oracle, x, vec_ids, raw[j], k, keep))
        j += 1
    return out, {"searched": int(valid.sum()), "candidates": int(n_cand), "scored": int(n_scored)}


def ivf_expected(oracle, table, x, vec_ids, triples, k, n_cand, W, sentinel=1000.0, found_rule=0):
    valid, raw, unit = build_queries(oracle, x, vec_ids, triples)
    lists = pm.ivf_lists(oracle, table, unit, n_cand, W, sentinel, found_rule) if len(unit) else np.empty((0, n_cand), np.int32)
    return expected(oracle, lists, valid, raw, x, vec_ids, triples, k) + (lists, raw, valid)


def pq_expected(oracle, table, x, vec_ids, triples, k, n_cand, subset_ids=None):
    valid, raw, unit = build_queries(oracle, x, vec_ids, triples)
    lists = pm.pq_lists(oracle, table, unit, n_cand, subset_ids) if len(unit) else np.empty((0, n_cand), np.int32)
    return expected(oracle, lists, valid, raw, x, vec_ids, triples, k) + (lists, raw, valid)


def analogy_loop(x, vec_ids, triple, list_ids):
    """host/freddy_udf.cpp analogy_common, literally: raw by two rounded binary32 operations per element, then over the list: skip
    ids < 0 and the inputs, skip ids without a vector, the binary32 chain scalar += raw[i] * v4[i], keep the best (ties: lowest id).
    Returns (id, similarity) or (-1, None)."""
    def vec(i):
        r = int(np.searchsorted(vec_ids, i))
        return x[r] if r < vec_ids.size and vec_ids[r] == i else None
    v1, v2, v3 = (vec(i) for i in triple)
    if v1 is None or v2 is None or v3 is None:
        return -1, None
    raw = ((v3 - v1).astype(np.float32) + v2).astype(np.float32)
    result, best, have = -1, np.float32(0), False
    for i in list_ids:
        if i < 0 or i in tuple(triple):
            continue
        v4 = vec(i)
        if v4 is None:
            continue
        s = np.float32(0.0)
        for a, b in zip(raw, v4):
            s = np.float32(s + np.float32(a * b))
        if not have or s > best or (s == best and i < result):
            have, best, result = True, s, int(i)
    return result, (best if have else None)


# ---- the main case's triples (tables: pv_model.main_tables(), 20 000 x 300 with rows 10000..10039 copies of rows 100..139) ----------
@functools.lru_cache(maxsize=None)
def main_triples():
    """200 triples of ids: random ones; (r, r2, c) with r, r2 of one cluster and c one of the three nearest other rows of a duplicated
    row, so that raw is close to v_c and the duplicated row and its copy are among the answers with equal similarity; triples that repeat an
    id (w1 == w3: raw is v2 exactly)."""
    x, ids, _, _, _ = pm.main_tables()
    N = x.shape[0]
    rng = np.random.default_rng(21)
    t = rng.choice(ids, (200, 3)).astype(np.int32)
    for j in range(40):                                  # rows 100 + j and N / 2 + j hold one vector
        sim = x @ x[100 + j]
        sim[[100 + j, N // 2 + j]] = -2.0
        for n, c in enumerate(np.argsort(-sim)[:3]):
            r = int(rng.integers(0, N))
            simr = x @ x[r]
            simr[r] = -2.0
            t[70 + 3 * j + n] = (ids[r], ids[int(np.argmax(simr))], ids[c])
    t[60:70, 2] = t[60:70, 0]                            # w1 == w3
    t[5] = (ids[7], ids[105], ids[7])                    # raw = the duplicated row 105 itself: its copy may answer
    return t
