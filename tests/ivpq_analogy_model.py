"""What the batched analogy over the kNN-join (freddy_gpu_ivpq_analogy; analogy_3cosadd_in_ivpq, freddy--0.0.1.sql:1383-1425) must
return, from the oracle alone -- approx_analogy_model's steps with another stage one:
  1. raw and unit rows of the triples whose three ids have a vector             (approx_analogy_model.build_queries),
  2. per pass of such triples ONE Oracle.ivpq_search_in over the pass's unit rows at k = n_cand; its ids are the lists,
  3. ids < 0 (the join's fillers), ids without a vector and the three inputs dropped, Oracle.exact_knn of RAW over the rest
                                                                                (approx_analogy_model.expected).
The pass rule is the library's: min(live triples, 8 M / n_cand) triples per pass, or option analogy_pass when that is smaller."""
import numpy as np

import approx_analogy_model as am


def pass_size(n_live, n_cand, analogy_pass=0):
    p = min(n_live, max(1, (8 << 20) // n_cand))
    return min(p, analogy_pass) if analogy_pass > 0 else p


def expected(oracle, table, x, vec_ids, triples, k, n_cand, target_ids, alpha, pvf, method, use_target_lists=True, confidence=0.8,
             double_threshold=10000000, analogy_pass=0):
    """-> (per-triple entries, the stats, lists [Q'][n_cand], raw [Q'][d], valid [Q], iterations per pass)"""
    valid, raw, unit = am.build_queries(oracle, x, vec_ids, triples)
    n = len(unit)
    lists, iters = np.empty((n, n_cand), np.int32), []
    step = pass_size(n, n_cand, analogy_pass) if n else 1
    for q0 in range(0, n, step):
        l, it = oracle.ivpq_search_in(table, unit[q0:q0 + step], n_cand, target_ids, alpha, pvf, method, use_target_lists=use_target_lists,
                                      confidence=confidence, double_threshold=double_threshold)
        lists[q0:q0 + step] = l["id"]
        iters.append(it)
    rows, stats = am.expected(oracle, lists, valid, raw, x, vec_ids, triples, k)
    return rows, stats, lists, raw, valid, iters
