"""A numpy model of freddy_gpu_cluster (include/freddy_gpu.h) on top of tests/assign_model.py: generic_cluster's k-means with the
draws supplied, the semantics of the header restated operation by operation.

    cluster(assign, vectors, kc, draws, rounds) -> dict(clusters int32[n], sim float32[n], centroids float32[kc][d], trace)

assign(centroids) -> (best int32[n], sim float32[n]) is one of assign_model.exact_assign / pq_assign bound to its tables and tokens
(exact() and pq() below do that); vectors[i] is the row of the token at position i.  trace holds one record per draw of a cluster that
sampled: (round J, cluster I 0-based, t, x, len, position or -1 where x lies beyond the members), and one (J, I, -1, 0, 0, -1) for a
cluster whose ten draws were skipped because lens == 0.  members holds (J, I, |members|, len) of every cluster that sampled: a stale
member -- claimed in an earlier round, by no centroid in this one -- makes |members| > len."""
import numpy as np

import assign_model as am

SAMPLES = 10


def pick(upper, r):
    """min(max(rint(r * upper + 0.5), 1), upper) in binary64, the product rounded before the sum, rint half to even."""
    with np.errstate(all="ignore"):
        v = np.rint(np.float64(r) * np.float64(upper) + np.float64(0.5))
    if not v >= 1.0:
        return 1
    return int(upper) if v > upper else int(v)


def n_draws(kc, rounds):
    return kc + SAMPLES * kc * (rounds - 1)


def cluster(assign, vectors, kc, draws, rounds=10):
    vectors = np.ascontiguousarray(vectors, np.float32)
    draws = np.asarray(draws, np.float64)
    n, d = vectors.shape
    assert draws.size >= n_draws(kc, rounds) and not np.isnan(draws[:n_draws(kc, rounds)]).any()
    centroids = np.stack([vectors[pick(n, draws[i]) - 1] for i in range(kc)]).astype(np.float32)
    clusters, lens = np.zeros(n, np.int32), np.zeros(kc, np.int64)
    trace, sizes = [], []
    sim = np.full(n, am.NEG_INF, np.float32)
    for J in range(1, rounds + 1):
        best, sim = assign(centroids)
        claimed = best >= 0
        clusters[claimed] = best[claimed] + 1
        lens += np.bincount(best[claimed], minlength=kc)
        if J == rounds:
            break
        for i in range(kc):
            base = kc + ((J - 1) * kc + i) * SAMPLES
            if lens[i] == 0:
                trace.append((J, i, -1, 0, 0, -1))
                continue
            members = np.flatnonzero(clusters == i + 1)
            sizes.append((J, i, int(members.size), int(lens[i])))
            samples = []
            for t in range(SAMPLES):
                x = pick(int(lens[i]), draws[base + t])
                pos = int(members[x - 1]) if x <= members.size else -1
                trace.append((J, i, t, x, int(lens[i]), pos))
                if pos >= 0:
                    samples.append(vectors[pos])
            if samples:
                ns = np.float32(len(samples))
                c = np.zeros(d, np.float32)
                with np.errstate(all="ignore"):
                    for row in samples:
                        q = row / ns                      # float32 / float32: correctly rounded
                        c = c + q
                assert c.dtype == np.float32
                centroids[i] = c
            lens[i] = 0
    return dict(clusters=clusters, sim=np.asarray(sim, np.float32), centroids=centroids, trace=trace, members=sizes)


def token_vectors(table_ids, x, token_ids):
    r = am.rows_of(table_ids, token_ids)
    assert (r >= 0).all(), "the model takes tokens with a vector only (an unknown id is a refusal)"
    return np.asarray(x, np.float32)[r]


def exact(table_ids, x, token_ids, kc, draws, rounds=10):
    return cluster(lambda c: am.exact_assign(table_ids, x, c, token_ids), token_vectors(table_ids, x, token_ids), kc, draws, rounds)


def pq(oracle, table_ids, x, codebook, pq_ids, codes, token_ids, kc, draws, rounds=10, sentinel=1000.0):
    return cluster(lambda c: am.pq_assign(oracle, codebook, pq_ids, codes, c, token_ids, sentinel=sentinel),
                   token_vectors(table_ids, x, token_ids), kc, draws, rounds)


def same(got, exp):
    """(clusters, sim, centroids) of the device against the model's dict: clusters equal, sim and centroid bits equal with every NaN
    as 'a NaN'."""
    gc, gs, gm = got
    if not np.array_equal(gc, exp["clusters"]):
        return False
    for g, e in ((gs, exp["sim"]), (gm, exp["centroids"])):
        g, e = np.asarray(g, np.float32), np.asarray(e, np.float32)
        nan = np.isnan(e)
        if g.shape != e.shape or not np.array_equal(np.isnan(g), nan) or not np.array_equal(g[~nan].view(np.uint32), e[~nan].view(np.uint32)):
            return False
    return True
