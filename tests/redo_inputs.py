"""Degenerate inputs for the redo paths of the exact filter + refine design (exact2.h, analogy.h, exact_join.h; the host side in
exact.hip and exact_host.h), shared by tests/test_redo_inputs_cpu.py (which proves on the CPU that they are what they claim to be) and
tests/test_gpu_redo_paths.py (which runs them).  Inputs and expected lists only: nothing here touches a device.

The table: 20 000 x 300 rows of util.corpus with rows 5000 .. 14999 overwritten by row 4999 -- 10 001 equal rows, more than the
8 192 rows a candidate buffer holds, in a table just large enough for that (the buffer is min(N, 8192) rows).  Ids ascend with
gaps (2 row + 5: every id is odd, so an even number is an unknown id).

HOT inputs overflow the buffer for certain: every copy has one approximate score, so either all of them are candidates or
none, and the threshold is never above the copies' score when they tie for the best exact one.
  * the query x[4999]: every copy has similarity |x|^2, the table's largest;
  * the analogy (a, a, r), r a copy: 3CosAdd's raw vector is (v_r - v_a) + v_a ~ v_r, and 3CosMul's c1 = c2 makes the score
    grow with c3 alone; the 10 000 copies that are not the input r tie for the best score.
HEALTHY inputs are drawn from the rows below 4999 and stay far from the copies: their k-th best score at k = 32 exceeds the
copies' score by 0.05, hundreds of times the filter's bracket (EXF_EPS X |q| <= 6e-5 on this normalised table), so no copy is
a candidate of theirs.  test_redo_inputs_cpu.py asserts both statements with analogy_model and the oracle."""
import functools

import numpy as np

import analogy_model as am
import util

N, D = 20000, 300
ORIGINAL = 4999                                   # the row that is copied ...
COPY_ROWS = np.arange(4999, 15000)                # ... and every row that holds its vector (itself included)
CAP = 8192                                        # rows of a candidate buffer (exact_host.h: filter_plan)
K_MAX = 32                                        # the filter's largest k
GAP = 0.05
UNKNOWN_IDS = (4, 10**8, -7)

HOT_TRIPLES = ((7, 7, 4999), (9, 9, 6000), (13, 13, 4999))     # (w1, w2, w3) as table rows; the second: w3 is a copy, row 4999 stays a candidate
NEAR_MISS = (11, 12, 4999)                        # w1 != w2: the copies do not win, the triple is healthy (asserted on the CPU)
N_LIVE = 70                                       # passes of 32, 32 and 6 analogies; queries: a pass of 64 (two MFMA tiles) and one of 6
UNKNOWN_AT = (2, 35, 71)                          # caller positions of the triples with an unknown id (Q = 73)


@functools.lru_cache(maxsize=None)
def table():
    """(x[N][D] float32, ids[N] int32), read-only."""
    x = util.corpus(N).numpy().copy()             # (util.corpus is cached: never write into the shared table)
    x[5000:15000] = x[ORIGINAL]
    ids = (np.arange(N) * 2 + 5).astype(np.int32)
    x.setflags(write=False)
    ids.setflags(write=False)
    return x, ids


# ---- analogies ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def healthy_triples():
    """[N_LIVE][3] table rows below 4999; the near-miss replaces the triple at position 3 (pass 0 wherever nothing hot is put)."""
    t = np.random.default_rng(3).integers(0, ORIGINAL, size=(N_LIVE, 3))
    t[3] = NEAR_MISS
    t.setflags(write=False)
    return t


def analogy_call(hot, unknown_at=UNKNOWN_AT):
    """One call's triples.  hot: {position among the LIVE triples (the numbering the passes are cut in): row triple}; every other
    live triple is the healthy one of that position.  Triples with an unknown id are inserted at the caller positions
    unknown_at.  -> dict: triples [Q][3] ids, rows [N_LIVE][3] table rows of the live triples, live [N_LIVE] caller positions."""
    _, ids = table()
    rows = healthy_triples().copy()
    for p, t in hot.items():
        rows[p] = t
    Q = N_LIVE + len(unknown_at)
    live = np.array([q for q in range(Q) if q not in unknown_at])
    triples = np.empty((Q, 3), np.int32)
    triples[live] = ids[rows]
    for j, q in enumerate(unknown_at):
        triples[q] = ids[healthy_triples()[q % N_LIVE]]
        triples[q, j % 3] = UNKNOWN_IDS[j % len(UNKNOWN_IDS)]        # (each member of a triple is the unknown one once)
    return dict(triples=triples, rows=rows, live=live)


@functools.lru_cache(maxsize=None)
def analogy_lists(method):
    """{row triple: (ids[K_MAX], scores[K_MAX])} from ONE analogy_model.model call over every triple this module hands out.
    A shorter list is a prefix (ORDER BY score DESC, id ASC is a total order)."""
    x, ids = table()
    every = [tuple(t) for t in healthy_triples().tolist()] + list(HOT_TRIPLES)
    mi, ms = am.model(x, ids, ids[np.array(every)], K_MAX, method)
    return {t: (mi[j], ms[j]) for j, t in enumerate(every)}


def analogy_expected(call, k, method):
    """(ids[Q][k], scores[Q][k]) of analogy_model.model for the call: (-1, -inf) where an id is unknown."""
    lists = analogy_lists(method)
    Q = call["triples"].shape[0]
    ei = np.full((Q, k), -1, np.int32)
    es = np.full((Q, k), -np.inf, np.float64)
    for q, t in zip(call["live"], call["rows"].tolist()):
        ei[q], es[q] = lists[tuple(t)][0][:k], lists[tuple(t)][1][:k]
    return ei, es


def lowest_copy_ids(triple, k):
    """The k lowest ids of copies that are not inputs of the triple: a hot triple's answer."""
    _, ids = table()
    return ids[np.setdiff1d(COPY_ROWS, np.array(triple))[:k]]


# ---- queries --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def healthy_query_rows():
    rows = np.random.default_rng(4).choice(ORIGINAL, N_LIVE, replace=False)
    rows.setflags(write=False)
    return rows


def hot_query():
    return table()[0][ORIGINAL].copy()


def bad_query(q, kind):
    """q with one component replaced: a NaN, an Inf, or 3.2e38 -- finite, but over the 3e38 limit of exf_prep_kernel."""
    q = np.array(q, np.float32)
    q[17] = {"nan": np.nan, "inf": np.inf, "big": np.float32(3.2e38)}[kind]
    return q


def queries(Q=N_LIVE, hot_at=(), bad=None):
    """[Q][D]: the healthy queries with the hot query (bad = None) or bad_query(healthy query, bad) at the positions hot_at."""
    qs = table()[0][healthy_query_rows()[:Q]].copy()
    for i in hot_at:
        qs[i] = hot_query() if bad is None else bad_query(qs[i], bad)
    return qs


# ---- join ------------------------------------------------------------------------------------------------------------------
JOIN_Q = 200
JOIN_HOT_AT = (6, 127, 128, 199)                  # tile 0, the last query of tile 0, the first of tile 1, the last of its tail (tiles of 128)


def overflow_targets():
    """12 000 known ids that hold every copy, and two unknown ones (the targets of test_gpu_exact_join's overflow test)."""
    _, ids = table()
    return np.concatenate([ids[4000:16000], np.array([4, -7], np.int32)])


@functools.lru_cache(maxsize=None)
def healthy_targets():
    """9 000 ids of rows that are no copies (above the join's threshold of 8 000 known targets), shuffled, and two unknown ones."""
    _, ids = table()
    rng = np.random.default_rng(5)
    rows = rng.choice(np.setdiff1d(np.arange(N), COPY_ROWS), 9000, replace=False)
    t = rng.permutation(np.concatenate([ids[rows], np.array([4, -7], np.int32)])).astype(np.int32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def join_query_rows():
    """JOIN_Q rows below 4999 for the join over overflow_targets(), which holds only 1 999 rows that are no copies: a query drawn
    at random can have its 32nd best of those no better than the copies.  Rows are drawn once and kept, in drawing order, while
    their 32nd best similarity over the targets (float64 here; the CPU test measures it again with the oracle) exceeds the copies'
    by twice GAP."""
    x, _ = table()
    x64 = x.astype(np.float64)
    drawn = np.random.default_rng(6).choice(ORIGINAL, 400, replace=False)
    s = x64[4000:16000] @ x64[drawn].T
    kth = -np.sort(-s, axis=0)[K_MAX - 1]
    keep = drawn[kth - s[ORIGINAL - 4000] >= 2 * GAP][:JOIN_Q]
    assert keep.size == JOIN_Q
    keep.setflags(write=False)
    return keep


def join_queries():
    """[JOIN_Q][D]: healthy queries, the hot one at JOIN_HOT_AT."""
    qs = table()[0][join_query_rows()].copy()
    for i in JOIN_HOT_AT:
        qs[i] = hot_query()
    return qs
