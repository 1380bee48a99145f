"""Shared builders of small seeded tables for the parity tests (inputs only -- both the
oracle and the HIP path read exactly these arrays)."""
import functools

import numpy as np
import torch

from freddy_amd import index_build as ib


@functools.lru_cache(maxsize=None)
def corpus(N=20000, d=300, seed=11, dup_frac=0.01):
    torch.manual_seed(0)
    return ib.make_corpus(N, d=d, seed=seed, n_clusters=200, dup_frac=dup_frac, device="cpu")


@functools.lru_cache(maxsize=None)
def ivf_tables(N=20000, C=32, m=12, K=256, seed=5):
    x = corpus(N)
    return ib.build_ivf_index(x, C=C, m=m, K=K, train_size=min(N, 5000), iters=4, seed=seed)


@functools.lru_cache(maxsize=None)
def pq_tables(N=20000, m=12, K=256, seed=6):
    x = corpus(N)
    return ib.build_pq_index(x, m=m, K=K, train_size=min(N, 5000), iters=4, seed=seed)


@functools.lru_cache(maxsize=None)
def ivpq_tables(N=20000, m=30, K=32, k_coarse=8, seed=7):
    x = corpus(N)
    return ib.build_ivpq_index(x, m=m, K=K, k_coarse=k_coarse, train_size=min(N, 5000), iters=4, seed=seed)


# ---- tables of other shapes (tests/test_gpu_shapes.py, the odd-shape cases of tests/test_oracle.py) ----
@functools.lru_cache(maxsize=None)
def shape_corpus(N, d, seed=0):
    """N x d rows like corpus() in a latent space of min(10, d) dimensions, 1 % of them copies of other rows (ties)."""
    torch.manual_seed(0)
    return ib.make_corpus(N, d=d, seed=1000 + 7 * d + seed, n_clusters=120, latent=min(10, d), dup_frac=0.01, device="cpu")


@functools.lru_cache(maxsize=None)
def shape_pq_tables(d, m, K, N, seed=6):
    return ib.build_pq_index(shape_corpus(N, d), m=m, K=K, train_size=min(N, 5000), iters=3, seed=seed)


@functools.lru_cache(maxsize=None)
def shape_ivf_tables(d, m, K, C, N, seed=5):
    return ib.build_ivf_index(shape_corpus(N, d), C=C, m=m, K=K, train_size=min(N, 5000), iters=3, seed=seed)


@functools.lru_cache(maxsize=None)
def shape_ivpq_tables(d, m, K, k_coarse, N, seed=7):
    return ib.build_ivpq_index(shape_corpus(N, d), m=m, K=K, k_coarse=k_coarse, train_size=min(N, 5000), iters=3, seed=seed)


def shape_queries(N, d, Q, seed=7):
    """Q rows of shape_corpus(N, d) as queries (float32 copies)."""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(N, size=Q, replace=False))
    return shape_corpus(N, d)[torch.from_numpy(rows)].numpy().astype(np.float32)


def queries_from_corpus(N, Q, seed=7):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(1, N + 1), size=Q, replace=False)).astype(np.int32)
    x = corpus(N)
    return ids, x[torch.from_numpy(ids.astype(np.int64) - 1)].numpy().astype(np.float32)


def assert_same_lists(got_ids, got_dist, exp, what=""):
    """bit-exact (id, rank) and bit-exact float distance."""
    exp_ids = exp["id"].reshape(got_ids.shape)
    exp_d = exp["dist"].reshape(got_dist.shape)
    bad = np.argwhere(exp_ids != got_ids)
    assert bad.size == 0, f"{what}: id mismatch at {bad[:5].tolist()} exp {exp_ids[tuple(bad[0])]} got {got_ids[tuple(bad[0])]}"
    assert np.array_equal(exp_d.view(np.uint32), got_dist.view(np.uint32)), f"{what}: distance bits differ"


def assert_exact_lists(gi, gs, exp, k, what=""):
    """Exact kNN: exp[q] is the oracle's list of query q with at least k entries, or with every row there is (ORDER BY similarity
    DESC, id ASC is a total order: the list for k is the prefix).  Ids and similarity bits; (-1, -inf) behind the last row."""
    for qi, e in enumerate(exp[:gi.shape[0]]):
        e = e[:k]
        n = len(e)
        assert gi[qi, :n].tolist() == e["id"].tolist(), (what, qi)
        assert np.array_equal(gs[qi, :n].view(np.uint32), e["dist"].view(np.uint32)), (what, qi)
        assert (gi[qi, n:] == -1).all() and np.isneginf(gs[qi, n:]).all(), (what, qi)


# ---- non-finite inputs (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py) ----
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]     # a quiet NaN with the sign bit set
QUERY_POISONS = ("nan", "neg_nan", "pos_inf", "neg_inf", "both_inf", "all_nan")


def poison_query(q, kind, m, rng, where="first"):
    """A copy of q with the poison `kind`: the component is drawn by rng inside the first or the last of the m sub-vectors
    (`where`); both_inf puts +Inf into the first and -Inf into the last."""
    q = np.array(q, np.float32)
    d = q.size
    s = d // m
    first, last = int(rng.integers(0, s)), d - s + int(rng.integers(0, s))
    at = first if where == "first" else last
    if kind == "nan":
        q[at] = np.nan
    elif kind == "neg_nan":
        q[at] = NEG_NAN
    elif kind == "pos_inf":
        q[at] = np.inf
    elif kind == "neg_inf":
        q[at] = -np.inf
    elif kind == "both_inf":
        q[first], q[last] = np.inf, -np.inf
    elif kind == "all_nan":
        q[:] = np.nan
    else:
        raise ValueError(kind)
    return q


PLACEMENTS = ("every8", "run64", "ends")


def poisoned_rows(Q, placement, seed=0):
    """Indices of the poisoned queries of a batch of Q >= 128: one in every group of 8, the aligned run [64, 128), or both ends."""
    rng = np.random.default_rng(seed)
    if placement == "every8":
        return np.array([g + int(rng.integers(0, min(8, Q - g))) for g in range(0, Q, 8)])
    if placement == "run64":
        assert Q >= 128
        return np.arange(64, 128)
    if placement == "ends":
        return np.array([0, Q - 1])
    raise ValueError(placement)


def poison_batch(qs, placement, m, seed=0):
    """(poisoned copy of qs, bool mask of the poisoned rows).  The poisoned rows cycle through QUERY_POISONS, alternating
    between the first and the last sub-vector, so every batch holds every kind at both ends (from six poisoned rows on)."""
    rng = np.random.default_rng(1000 + seed)
    out = np.array(qs, np.float32)
    rows = poisoned_rows(out.shape[0], placement, seed)
    for j, r in enumerate(rows):
        kind = QUERY_POISONS[j % len(QUERY_POISONS)]
        out[r] = poison_query(out[r], kind, m, rng, where="first" if (j // len(QUERY_POISONS)) % 2 == 0 else "last")
    mask = np.zeros(out.shape[0], bool)
    mask[rows] = True
    return out, mask


def assert_rows_bit_equal(a, b, rows, what=""):
    """(ids, floats) pairs a and b agree bit for bit on `rows` (the cross-contamination check: no oracle involved)."""
    (ai, ad), (bi, bd) = a, b
    assert np.array_equal(ai[rows], bi[rows]), f"{what}: a healthy query's ids changed with its neighbours' poison"
    assert np.array_equal(ad[rows].view(np.uint32), bd[rows].view(np.uint32)), f"{what}: a healthy query's distances changed with its neighbours' poison"
