"""A numpy restatement of the similarities by row id (include/freddy_gpu.h: freddy_gpu_similarity_pairs / _matrix / _join): what the
GPU tests compare with, bit for bit.  The chain is an explicit float32 loop over the dimensions (vectorised over the pairs only),
held to Oracle.cosine_similarity_bytea in tests/test_similarity_inputs_cpu.py; the predicate of the join is PostgreSQL's float4gt."""
import numpy as np


def chain(a, b):
    """scalar = 0; scalar += v1[i] * v2[i], i ascending, every product and every sum rounded to binary32 (core_functions.c:67-81).
    a, b: float32 arrays whose last axis is the dimension; the others broadcast."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, np.float32)
    with np.errstate(all="ignore"):
        for i in range(a.shape[-1]):
            p = a[..., i] * b[..., i]          # float32 * float32 -> float32: rounded once
            acc = acc + p                      # and the sum once
    return acc


def float4gt(a, b):
    """PostgreSQL's float4 `a > b` (float4_cmp_internal): NaN = NaN, NaN > every non-NaN, -0.0 = +0.0."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        plain = a > b
    return np.where(an, ~bn, np.where(bn, False, plain))


# (a, b, a > b) -- the cases the predicate is checked against, written down by hand
NAN, NNAN, INF = np.float32(np.nan), np.array([0xffc00000], np.uint32).view(np.float32)[0], np.float32(np.inf)
GT_CASES = [
    (NAN, 1.0, True), (NNAN, 1.0, True), (NAN, INF, True), (NAN, -INF, True), (NAN, NAN, False), (NNAN, NAN, False), (NAN, NNAN, False),
    (1.0, NAN, False), (INF, NAN, False), (-INF, NAN, False), (0.0, NAN, False),
    (0.0, -0.0, False), (-0.0, 0.0, False), (0.0, 0.0, False), (-0.0, -0.0, False),
    (INF, 1.0, True), (INF, INF, False), (INF, -INF, True), (-INF, INF, False), (-INF, -INF, False), (1.0, INF, False), (1.0, -INF, True),
    (1.0, 1.0, False), (np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0, True), (1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), False),
    (1e-45, 0.0, True), (-1e-45, -0.0, False), (0.0, -1e-45, True),
]


def rows_of(table_ids, ids):
    """the row of every id in a table of ascending ids, -1 where it has none"""
    table_ids, ids = np.asarray(table_ids, np.int64), np.asarray(ids, np.int64).reshape(-1)
    if table_ids.size == 0:
        return np.full(ids.size, -1, np.int64)
    pos = np.minimum(np.searchsorted(table_ids, ids), table_ids.size - 1)
    return np.where(table_ids[pos] == ids, pos, -1)


def pairs(table_ids, x, ids_a, ids_b):
    """-> (sim[n] float32, known[n] bool)"""
    ra, rb = rows_of(table_ids, ids_a), rows_of(table_ids, ids_b)
    known = (ra >= 0) & (rb >= 0)
    sim = np.zeros(ra.size, np.float32)
    if known.any():
        sim[known] = chain(x[ra[known]], x[rb[known]])
    return sim, known


def _a_side(table_ids, x, a):
    a = np.asarray(a)
    if np.issubdtype(a.dtype, np.integer):
        r = rows_of(table_ids, a)
        v = np.zeros((r.size, x.shape[1]), np.float32)
        v[r >= 0] = x[r[r >= 0]]
        return v, r >= 0
    v = np.asarray(a, np.float32)
    return v, np.ones(v.shape[0], bool)


def matrix(table_ids, x, a, b_ids):
    """a: integer ids or float vectors [na][d] -> (out[na][nb] float32, known_a[na], known_b[nb]); v1 is the A row"""
    va, ka = _a_side(table_ids, x, a)
    rb = rows_of(table_ids, b_ids)
    kb = rb >= 0
    out = np.zeros((va.shape[0], rb.size), np.float32)
    ia, ib = np.flatnonzero(ka), np.flatnonzero(kb)
    if ia.size and ib.size:
        out[np.ix_(ia, ib)] = chain(va[ia][:, None, :], x[rb[ib]][None, :, :])
    return out, ka, kb


def join_of(out, ka, kb, threshold, max_pairs=None):
    """the join over a matrix: (ia, ib, sim, total), i ascending then j ascending, the first max_pairs of them"""
    mask = ka[:, None] & kb[None, :] & float4gt(out, np.float32(threshold))
    ia, ib = np.nonzero(mask)                  # row-major: i ascending, then j ascending
    total = ia.size
    n = total if max_pairs is None else min(total, max_pairs)
    return ia[:n].astype(np.int32), ib[:n].astype(np.int32), out[ia[:n], ib[:n]], total


def join(table_ids, x, a, b_ids, threshold, max_pairs=None):
    return join_of(*matrix(table_ids, x, a, b_ids), threshold, max_pairs)


def same_floats(got, exp):
    """bit for bit, except that a NaN is any NaN (as tests/util.py treats the payloads)"""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    if got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en]))


def assign_of(out, kb):
    """the column argmax of a matrix under freddy_gpu_exact_assign's rule: similarity DESC in float4 order (every NaN the one largest
    value), A index ASC -> (query[nb], sim[nb]); (-1, -inf) for an unknown B"""
    nb = out.shape[1]
    q, s = np.full(nb, -1, np.int32), np.full(nb, -np.inf, np.float32)
    for j in np.flatnonzero(kb):
        best = -1
        for i in range(out.shape[0]):
            if best < 0 or float4gt(out[i, j], out[best, j]):
                best = i
        q[j], s[j] = best, out[best, j]
    return q, s
