"""numpy model of analogy_pair_direction (postgres-word2vec_amd/csrc/analogy.h; freddy--0.0.1.sql:1212-1229).

score(v4) = cosine_similarity_bytea(vec_normalize_bytea(vec_minus_bytea(v1, v2)), vec_normalize_bytea(vec_minus_bytea(v3, v4))),
every step a binary32 operation as core_functions.c does it: the chains are loops over d on np.float32 arrays (NumPy 2's NEP 50
casting never widens them), np.sqrt on float32 (correctly rounded, equal to (float)sqrt((double)x) for every float) and float32
division.  0/0 and x/NaN are not errors here: such a row scores NaN, and analogy_model.topk sorts NaN first."""
import numpy as np

import analogy_model as am


def normalize(t):
    """vec_normalize_bytea of every row of t [Q][d] (core_functions.c:243-269)."""
    t = np.asarray(t, np.float32)
    sq = np.zeros(t.shape[0], np.float32)
    for i in range(t.shape[1]):
        sq = sq + t[:, i] * t[:, i]
    length = np.sqrt(sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t / length[:, None]


def scores(x, x_t, triples):
    """[Q][N] float64 (the binary32 score widened) of every row for every (row-position) triple; x_t = the table transposed."""
    x = np.asarray(x, np.float32)
    t = np.asarray(triples).reshape(-1, 3)
    d, n = x_t.shape
    a = normalize(x[t[:, 0]] - x[t[:, 1]])              # [Q][d], once per analogy
    v3 = x[t[:, 2]]
    sq = np.zeros((t.shape[0], n), np.float32)
    for i in range(d):
        df = v3[:, i:i + 1] - x_t[i][None, :]
        sq = sq + df * df
    length = np.sqrt(sq)
    s = np.zeros((t.shape[0], n), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(d):
            df = v3[:, i:i + 1] - x_t[i][None, :]
            u = df / length
            s = s + a[:, i:i + 1] * u
    assert s.dtype == np.float32 and sq.dtype == np.float32 and a.dtype == np.float32
    return s.astype(np.float64)


def model(x, ids, triples_ids, k, subset_ids=None, x_t=None):
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
    sc = scores(x, x_t, tr)
    for j, q in enumerate(live):
        out_i[q], out_s[q] = am.topk(sc[j], ids, set(tr[j].tolist()), k, rows)
    return out_i, out_s
