"""numpy model of the exact analogies (postgres-word2vec_amd/csrc/analogy.h; freddy--0.0.1.sql:1231-1315).

cos(a, b) is cosine_similarity_bytea: the binary32 chain s += a[i] * b[i], i ascending, each operation rounded -- np.float32
arrays and np.float32 scalars throughout, so NumPy 2's NEP 50 casting never widens it.  3CosMul is float8 (PostgreSQL's
float48pl): the reading analogy.h documents, written down here a second time as the test's model."""
import numpy as np


def chains(vecs, x_t):
    """[m][N] float32: cosine_similarity_bytea(vecs[j], row) for every row; x_t = the table transposed, [d][N] float32."""
    vecs = np.asarray(vecs, np.float32).reshape(-1, x_t.shape[0])
    s = np.zeros((vecs.shape[0], x_t.shape[1]), np.float32)
    for i in range(x_t.shape[0]):
        s = s + vecs[:, i:i + 1] * x_t[i][None, :]
    return s


def raw_3cosadd(v1, v2, v3):
    """vec_plus_bytea(vec_minus_bytea(v3, v1), v2), elementwise binary32."""
    return (np.asarray(v3, np.float32) - np.asarray(v1, np.float32)) + np.asarray(v2, np.float32)


def mul_score(c1, c2, c3):
    """((c3 + 1)/2) * ((c2 + 1.0)/2.0) / (((c1 + 1.0)/2.0) + 0.001) in float8, c_i the binary32 cosines widened."""
    a = (np.asarray(c3, np.float64) + 1.0) / 2.0
    b = (np.asarray(c2, np.float64) + 1.0) / 2.0
    d = (np.asarray(c1, np.float64) + 1.0) / 2.0 + 0.001
    return (a * b) / d


def scores(x, x_t, triples, method):
    """[Q][N] float64 scores of every row for every (row-position) triple."""
    t = np.asarray(triples).reshape(-1, 3)
    if method == "3cosadd":
        raw = raw_3cosadd(x[t[:, 0]], x[t[:, 1]], x[t[:, 2]])
        return chains(raw, x_t).astype(np.float64)
    c = chains(x[t.ravel()], x_t).reshape(t.shape[0], 3, -1)
    return mul_score(c[:, 0], c[:, 1], c[:, 2])


def topk(score, ids, exclude_rows, k, rows=None):
    """ORDER BY score DESC, id ASC over `rows` (all when None) minus the excluded rows; (ids[k], scores[k]) padded with
    (-1, -inf).  NaN sorts first (PostgreSQL's float8 order; reported as the canonical quiet NaN), -0 counts as +0 (and is
    reported so)."""
    n = score.shape[0]
    ok = np.zeros(n, bool)
    if rows is None:
        ok[:] = True
    else:
        ok[np.asarray(rows, np.int64)] = True
    ok[np.asarray(list(exclude_rows), np.int64)] = False
    cand = np.nonzero(ok)[0]
    s = score[cand] + 0.0
    nan = np.isnan(s)
    s[nan] = np.nan
    order = np.lexsort((ids[cand], -np.where(nan, 0.0, s), ~nan))[:k]   # (last key first: NaN, then score DESC, then id)
    out_i = np.full(k, -1, np.int32)
    out_s = np.full(k, -np.inf, np.float64)
    out_i[:order.size] = ids[cand[order]]
    out_s[:order.size] = s[order]
    return out_i, out_s


def model(x, ids, triples_ids, k, method, subset_ids=None, x_t=None):
    """The whole contract: triples of ids -> (ids[Q][k], scores[Q][k]); unknown input ids give an all-(-1, -inf) row."""
    x = np.asarray(x, np.float32)
    ids = np.asarray(ids, np.int32)
    if x_t is None:
        x_t = np.ascontiguousarray(x.T)
    pos = {int(v): i for i, v in enumerate(ids)}
    rows = None
    if subset_ids is not None:
        rows = sorted({pos[int(v)] for v in subset_ids if int(v) in pos})
    T = np.asarray(triples_ids).reshape(-1, 3)
    out_i = np.full((T.shape[0], k), -1, np.int32)
    out_s = np.full((T.shape[0], k), -np.inf, np.float64)
    live = [q for q in range(T.shape[0]) if all(int(v) in pos for v in T[q])]
    if not live:
        return out_i, out_s
    tr = np.array([[pos[int(v)] for v in T[q]] for q in live])
    sc = scores(x, x_t, tr, method)
    for j, q in enumerate(live):
        out_i[q], out_s[q] = topk(sc[j], ids, set(tr[j].tolist()), k, rows)
    return out_i, out_s
