"""A numpy model of the two assign contracts (include/freddy_gpu.h: freddy_gpu_exact_assign / freddy_gpu_pq_assign).

exact: per (target, query) the binary32 chain "scalar += q[j] * v[j]", j ascending -- vectorised over the pairs, a Python loop
over j, every product and every sum rounded to float32 -- then per target the first query under PostgreSQL's float4 order DESC
(a NaN above every number, all NaNs equal), query index ASC.
pq: per (target, query) the ADC sum over the positions in order of the oracle's LUT entries, candidates by the strict
"dist < sentinel", key = (1.0 - emit_roundtrip(dist) / 2.0)::float4 through the oracle's text round trip (as
test_gpu_udf._sim_of), first under key DESC, query index ASC.
Both return (query index int32[n], similarity float32[n]), positional, (-1, -inf) where there is nothing."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def pg_ord(x):
    """float32 array -> uint32 that ascends with PostgreSQL's float4 order; every NaN maps to the one largest value, nothing to 0."""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32)
    o = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), o)


def rows_of(table_ids, target_ids):
    """Row of every target id in the ascending table_ids, -1 where it has none."""
    table_ids = np.asarray(table_ids, np.int32)
    t = np.asarray(target_ids, np.int32).reshape(-1)
    if table_ids.size == 0:
        return np.full(t.size, -1, np.int64)
    pos = np.searchsorted(table_ids, t)
    pos_c = np.minimum(pos, table_ids.size - 1)
    return np.where(table_ids[pos_c] == t, pos_c, -1).astype(np.int64)


def chain_sims(queries, rows):
    """[n][Q] float32: the chain of every (row, query) pair."""
    q = np.ascontiguousarray(queries, np.float32)
    v = np.ascontiguousarray(rows, np.float32)
    acc = np.zeros((v.shape[0], q.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for j in range(q.shape[1]):
            acc = acc + v[:, j:j + 1] * q[None, :, j]      # float32 * float32 and float32 + float32: one rounding each
    assert acc.dtype == np.float32
    return acc


def _first_best(ords, values):
    """ords [n][Q] uint32 (0 = not a candidate) -> (first argmax or -1, its value or -inf)."""
    n = ords.shape[0]
    best = np.argmax(ords, axis=1) if ords.shape[1] else np.zeros(n, np.int64)     # (the first of equal maxima)
    have = ords[np.arange(n), best] > 0 if ords.shape[1] else np.zeros(n, bool)
    out_q = np.where(have, best, -1).astype(np.int32)
    out_s = np.where(have, values[np.arange(n), best], NEG_INF).astype(np.float32)
    return out_q, out_s


def exact_assign(table_ids, vectors, queries, target_ids):
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, np.asarray(vectors).shape[1])
    r = rows_of(table_ids, target_ids)
    out_q = np.full(r.size, -1, np.int32)
    out_s = np.full(r.size, NEG_INF, np.float32)
    ok = np.flatnonzero(r >= 0)
    if ok.size and q.shape[0]:
        sims = chain_sims(q, np.asarray(vectors, np.float32)[r[ok]])
        out_q[ok], out_s[ok] = _first_best(pg_ord(sims), sims)
    return out_q, out_s


def adc_dists(oracle, codebook, codes_of_rows, queries):
    """[n][Q] float32: dist = 0 + lut[0][c0] + lut[1][c1] + ... with the oracle's LUT of every query."""
    cb = np.ascontiguousarray(codebook, np.float32)
    m, K, _ = cb.shape
    luts = np.stack([oracle.lut(q, cb).reshape(m, K) for q in np.ascontiguousarray(queries, np.float32)])   # [Q][m][K]
    codes = np.asarray(codes_of_rows).astype(np.int64)
    acc = np.zeros((codes.shape[0], luts.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for p in range(m):
            acc = acc + luts[:, p, codes[:, p]].T
    assert acc.dtype == np.float32
    return acc


def similarity_of(oracle, dists):
    """(1.0 - (distance / 2.0))::float4 of the emitted distance, elementwise (finite, non-negative distances)."""
    d = np.ascontiguousarray(dists, np.float32)
    uniq, inv = np.unique(d.view(np.uint32), return_inverse=True)
    vals = np.array([np.float32(1.0 - float(oracle.emit_roundtrip(u)) / 2.0) for u in uniq.view(np.float32)], np.float32)
    return vals[inv].reshape(d.shape)


def pq_assign(oracle, codebook, table_ids, codes, queries, target_ids, sentinel=1000.0):
    cb = np.ascontiguousarray(codebook, np.float32)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, cb.shape[0] * cb.shape[2])
    r = rows_of(table_ids, target_ids)
    out_q = np.full(r.size, -1, np.int32)
    out_s = np.full(r.size, NEG_INF, np.float32)
    ok = np.flatnonzero(r >= 0)
    if ok.size and q.shape[0]:
        dist = adc_dists(oracle, cb, np.asarray(codes)[r[ok]], q)
        with np.errstate(invalid="ignore"):
            cand = dist < np.float32(sentinel)            # (strict; false for a NaN)
        keys = np.full(dist.shape, NEG_INF, np.float32)
        keys[cand] = similarity_of(oracle, dist[cand])
        ords = np.where(cand, pg_ord(keys), np.uint32(0))
        out_q[ok], out_s[ok] = _first_best(ords, keys)
    return out_q, out_s


def first_per_token(rows, n):
    """The list-based definition: rows = [(similarity, qid 1-based, tid 1-based)] ORDER BY similarity DESC, qid, tid; the first row
    of every token -> (0-based query index or -1, similarity or -inf)."""
    out_q = np.full(n, -1, np.int32)
    out_s = np.full(n, NEG_INF, np.float32)
    for sim, qid, tid in sorted(rows, key=lambda r: (-r[0], r[1], r[2])):
        if out_q[tid - 1] < 0:
            out_q[tid - 1] = qid - 1
            out_s[tid - 1] = sim
    return out_q, out_s


def same(got, exp):
    """out_query equal, out_sim equal bit for bit with every NaN as 'a NaN'."""
    (gq, gs), (eq, es) = got, exp
    gs, es = np.asarray(gs, np.float32), np.asarray(es, np.float32)
    nan = np.isnan(es)
    return (np.array_equal(gq, eq) and np.array_equal(np.isnan(gs), nan)
            and np.array_equal(gs[~nan].view(np.uint32), es[~nan].view(np.uint32)))
