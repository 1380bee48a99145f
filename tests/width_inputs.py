"""Inputs of tests/test_gpu_selection_widths.py, which launches every WaveSelect<V> instantiation of every dispatch family at both
sides of its bounds, and of tests/test_width_inputs_cpu.py, which proves with the oracle alone that these cases reach what they
claim.  Tables, queries and case lists only: nothing here touches a device.

Every search path keeps its candidates in a WaveSelect<V> of 64 V keys and picks V from one ladder (csrc/generic.hip pick_V,
restated below): L <= 64 -> 1, <= 128 -> 2, <= 256 -> 4, <= 512 -> 8, <= 1024 -> 16.  What L is depends on the family:
  ivfadc12 / ivfadc0   adc_scan_kernel<12 | 0, V> + merge_replay_kernel<V> of the IVFADC generic path      L = 2k
  pq12 / pq0           the same kernels from the flat PQ scan                                               L = min(2k, 1024)
  probe                probe_plan_kernel<V>                                                                 L = 2W
  exact64 / exact300   exact_scan_kernel<V, QT> + exact_merge_kernel<V>                                     L = min(k, 1024)
  exact_join           the exact join's all-exact path (the same kernels; one k per width)                  L = k
  join_m01             join_query_kernel<V>, methods 0 and 1                                                L = 2k
  join_pv              join_query_kernel<V>, method 2                                                       L = k pvf
  side_sort            side_sort_kernel<V>                                                                  L = coarse_codes
  traverse             join_traverse_kernel<V[, SMALL]>                                                     L = coarse_codes^2
FAMILIES holds, per family, the case list, L of a case and the values L can take; coverage_gaps() computes from the LIST which
widths and which sides of which rung it reaches, so a case that is deleted shows up as a gap."""
import functools

import numpy as np

import util

RUNGS = (64, 128, 256, 512, 1024)
WIDTHS = (1, 2, 4, 8, 16)


def pick_V(L):
    """csrc/generic.hip pick_V: the selection width of a list of L keys; 0 = no instantiation."""
    for v, r in zip(WIDTHS, RUNGS):
        if L <= r:
            return v
    return 0


def _frozen(arrays):
    """read-only COPIES (the tables of util are cached and shared with other tests: never write into them or lock them)"""
    out = {name: np.array(a) for name, a in arrays.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the case lists ---------------------------------------------------------------------------------------------------------
K2 = (32, 33, 64, 65, 128, 129, 256, 257, 512, 513)                  # L = 2k: both sides of 64 .. 1024 (513: the selection passes of bigk.h)
PROBE_W = (32, 33, 64, 65, 128, 129, 256, 257, 512)                  # L = 2W (W = 513 is refused: test_gpu_parity)
EXACT_K = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)         # L = k (1025: passes of 1024 keys)
EXACT_JOIN_K = (64, 128, 256, 512, 1024)                             # one k per width
JOIN_K = (32, 33, 64, 65, 128, 129, 256, 257, 512)                   # methods 0 / 1 (k = 513 ..: test_gpu_join_bigk)
JOIN_PV = ((8, 8), (13, 5), (32, 4), (43, 3), (64, 4), (257, 1), (128, 4), (171, 3), (256, 4))   # (k, pvf): k pvf = 64|65 .. 512|513, 1024
SIDE_KC = (64, 65, 128, 129, 256, 257, 512, 513, 1024)               # coarse_codes (1025 is refused)
TRAVERSE_KC = (8, 9, 11, 12, 16, 17, 22, 23, 32)                     # cells = 64|81, 121|144, 256|289, 484|529, 1024

_EVEN = tuple(range(2, 1027, 2))
_ALL = tuple(range(1, 1026))
FAMILIES = {
    # name: (cases, L of a case, the values L can take in ascending order, is the first value above 1024 part of the family)
    "ivfadc12": (K2, lambda k: 2 * k, _EVEN, True),
    "ivfadc0": (K2, lambda k: 2 * k, _EVEN, True),
    "pq12": (K2, lambda k: 2 * k, _EVEN, True),
    "pq0": (K2, lambda k: 2 * k, _EVEN, True),
    "probe": (PROBE_W, lambda W: 2 * W, _EVEN[:-1], False),
    "exact64": (EXACT_K, lambda k: k, _ALL, True),
    "exact300": (EXACT_K, lambda k: k, _ALL, True),
    "join_m01": (JOIN_K, lambda k: 2 * k, _EVEN[:-1], False),
    "join_pv": (JOIN_PV, lambda c: c[0] * c[1], _ALL[:-1], False),
    "side_sort": (SIDE_KC, lambda kc: kc, _ALL[:-1], False),
    "traverse": (TRAVERSE_KC, lambda kc: kc * kc, tuple(i * i for i in range(2, 33)), False),
}


def coverage_gaps(name, cases=None):
    """What the case list of a family does NOT reach, as a list of sentences (empty: full coverage): every width; for every rung
    the largest L that stays at or below it and the smallest that crosses it (the top rung's crossing only where the family has
    a path beyond 1024 keys); one case whose L fills 64 V exactly."""
    listed, L_of, grid, beyond = FAMILIES[name]
    Ls = sorted({L_of(c) for c in (listed if cases is None else cases)})
    gaps = [f"{name}: V = {v} is never reached" for v in WIDTHS if v not in {pick_V(L) for L in Ls}]
    for r in RUNGS:
        below = max(g for g in grid if g <= r)
        if below not in Ls:
            gaps.append(f"{name}: L = {below}, the largest at or below {r}, is missing")
        above = [g for g in grid if g > r]
        if (r < 1024 or beyond) and (not above or above[0] not in Ls):
            gaps.append(f"{name}: the smallest L above {r} is missing")
    if not any(L == 64 * pick_V(L) for L in Ls):
        gaps.append(f"{name}: no case fills 64 V keys exactly")
    return gaps


# ---- A. IVFADC --------------------------------------------------------------------------------------------------------------
SHAPES = {"12": (300, 12, 256), "0": (64, 8, 16)}      # adc_scan_kernel<12, V> and <0, V>
IVF_C, IVF_FROM = 6, 14000
IVF_SIZES = (2300, 1500, 1100, 600, 350, 150)          # rows of the six lists, largest natural list first: 6000 rows
TIE_K = (32, 64, 128, 256, 512)                        # one k per width with more ties than keys kept
TIE_ROWS = 2 * 512 + 3                                 # rows of the tie group: 2k + 3 at the largest k


@functools.lru_cache(maxsize=None)
def ivf_table(key):
    """An IVF index over 6000 of 14 000 corpus rows: the first IVF_SIZES[j] rows of the j-th largest list of the index over all
    of them (lists of 150 .. 2300 rows: with W = 1 some queries finish in round one at every k and others carry their list over).
    Every other row of the largest list's first 2054 shares ONE code row: TIE_ROWS equal ADC distances per query, their ids
    interleaved with other rows' ids.  tie_query is the vector of the group's first row."""
    d, m, K = SHAPES[key]
    t = util.shape_ivf_tables(d, m, K, IVF_C, IVF_FROM)
    nat = np.diff(t["list_off"])
    order = np.argsort(-nat, kind="stable")
    size = np.empty(IVF_C, np.int64)
    size[order] = IVF_SIZES
    assert (size <= nat).all(), (size, nat)
    keep = np.concatenate([np.arange(t["list_off"][c], t["list_off"][c] + size[c]) for c in range(IVF_C)])
    ids, codes = t["ids"][keep].copy(), t["codes"][keep].copy()
    list_off = np.zeros(IVF_C + 1, np.int32)
    list_off[1:] = np.cumsum(size)
    pos = list_off[order[0]] + 2 * np.arange(TIE_ROWS)
    codes[pos] = codes[pos[0]]
    x = util.shape_corpus(IVF_FROM, d).numpy()
    out = dict(coarse=t["coarse"], codebook=t["codebook"], list_off=list_off, ids=ids, codes=codes, tie_pos=pos,
               tie_query=x[ids[pos[0]] - 1].copy(), vectors=x[ids - 1])
    return _frozen(out)


def ivf_pin_args(t):
    return (t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])


TIE_AT = 3                                             # position of the tie query in every batch of 8


def _with_tie(qs, tie):
    qs = np.array(qs, np.float32)
    qs[TIE_AT] = tie
    qs.setflags(write=False)
    return qs


@functools.lru_cache(maxsize=None)
def ivf_queries(key):
    d = SHAPES[key][0]
    return _with_tie(util.shape_queries(IVF_FROM, d, 8, seed=3), ivf_table(key)["tie_query"])


def _inner_sentinel(t, qs, nth):
    """A sentinel inside the data: the median over the queries of their nth smallest ADC distance to the table's rows, in float64
    (the CPU test asserts with the oracle that lists hold rows AND end in padding entries under it)."""
    cb = t["codebook"].astype(np.float64)
    m, K, S = cb.shape
    cell = np.repeat(np.arange(t["list_off"].size - 1), np.diff(t["list_off"]))
    codes = t["codes"].astype(np.int64)
    nths = []
    for q in qs.astype(np.float64):
        r = (q[None, :] - t["coarse"].astype(np.float64)).reshape(-1, m, 1, S)            # [C][m][1][S]
        lut = ((r - cb[None, :, :, :]) ** 2).sum(-1)                                     # [C][m][K]
        adc = lut[cell[:, None], np.arange(m)[None, :], codes].sum(1)
        nths.append(np.sort(adc)[nth])
    return float(np.float32(np.median(nths)))


@functools.lru_cache(maxsize=None)
def ivf_settings(key):
    """(found rule, sentinel) of every call: the reference's rule with its sentinel of 1000, the accepted-rows rule with a sentinel
    that about 20 rows per query stay under (the tie query's group does: its list is full)."""
    return ((0, 1000.0), (1, _inner_sentinel(ivf_table(key), ivf_queries(key), 20)))


IVF_W = (IVF_C, 1)
IVF_DEV_K = (128, 129)                                 # the rung that also goes through the device-pointer call


# ---- B. flat PQ -------------------------------------------------------------------------------------------------------------
PQ_N, PQ_TIE_FIRST, PQ_SENTINEL = 3000, 100, 100.0


@functools.lru_cache(maxsize=None)
def pq_table(key):
    """3000 rows; rows 100, 102, .., 2152 share the code row of row 100 (ids = row + 1 ascend: interleaved with the others)."""
    d, m, K = SHAPES[key]
    t = util.shape_pq_tables(d, m, K, PQ_N)
    codes = t["codes"].copy()
    pos = PQ_TIE_FIRST + 2 * np.arange(TIE_ROWS)
    codes[pos] = codes[PQ_TIE_FIRST]
    out = dict(codebook=t["codebook"], ids=t["ids"], codes=codes, tie_pos=pos,
               tie_query=util.shape_corpus(PQ_N, d).numpy()[PQ_TIE_FIRST].copy())
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def pq_queries(key):
    return _with_tie(util.shape_queries(PQ_N, SHAPES[key][0], 8, seed=4), pq_table(key)["tie_query"])


def pq_small_subset():
    """20 known rows (four of the tie group among them), two duplicates and two unknown ids: fewer rows than every k of K2."""
    return np.array(list(range(7, 2000, 125)) + [101, 103, 105, 107, 7, 101, PQ_N + 5, -3], np.int32)


# ---- C. probe plan ----------------------------------------------------------------------------------------------------------
PROBE_C, PROBE_K, PROBE_FAR = 520, 5, 6                # cells, k, position of the query far from every centroid
PROBE_EMPTY = (0, 77, 300, 519)                        # cells without rows
PROBE_DUP = ((5, 17), (300, 2), (3, 2))                # centroid [a] = centroid [b], bit for bit
PROBE_EDGE, PROBE_EDGE_W = 0, (32, 64, 128, 256, 512)  # the query with equally near cells at ranks W - 1 and W, and those W
PROBE_FEW_K = 400                                      # more than the rows of the cells the far query can reach (fewer rows than k)
CELL_LIMIT = 100.0                                     # freddy.c:266-283: a cell at this distance or beyond is never probed


def _nearest(a, b):
    """index of the row of b nearest to every row of a (float64; input construction only)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.argmin((a * a).sum(1)[:, None] - 2.0 * a @ b.T + (b * b).sum(1)[None, :], axis=1)


def _encode(cb, v):
    """PQ codes of v under the codebook cb[m][K][S] (float64 argmin; input construction only)"""
    m, K, S = cb.shape
    return np.stack([_nearest(v[:, p * S:(p + 1) * S], cb[p]) for p in range(m)], axis=1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def probe_table():
    """An IVF index of the (64, 8, 16) shape with 520 cells of at most 12 rows: the centroids are 520 corpus rows, a cell holds up
    to 2 .. 12 of the rows nearest to it (drawn per cell), four cells hold none, three centroids are copies of others, and five
    more are copies of the cell one rank nearer to query 0."""
    d, m, K = SHAPES["0"]
    x = util.shape_corpus(6000, d).numpy()
    rng = np.random.default_rng(41)
    first = x[rng.choice(6000, PROBE_C, replace=False)].copy()          # the centroids the rows are assigned and encoded with
    cell = _nearest(x, first)
    coarse = first.copy()
    for a, b in PROBE_DUP:
        coarse[a] = coarse[b]
    # ... and for query PROBE_EDGE the cell at rank W (from 0) becomes a copy of the one at rank W - 1, for every bound W of the
    # ladder: with W probes exactly one of two equally near cells is taken, with W + 1 both are
    q = probe_queries()[PROBE_EDGE].astype(np.float64)
    order = np.argsort(((coarse.astype(np.float64) - q[None, :]) ** 2).sum(1), kind="stable")
    for W in PROBE_EDGE_W:
        coarse[order[W]] = coarse[order[W - 1]]
    want = rng.integers(2, 13, size=PROBE_C)
    want[list(PROBE_EMPTY)] = 0
    rows = [np.nonzero(cell == c)[0][:want[c]] for c in range(PROBE_C)]
    for W in PROBE_EDGE_W:                                                # (the two lists differ in length: one row less where they do not)
        a, b = order[W - 1], order[W]
        if rows[a].size == rows[b].size:
            rows[b] = rows[b][:-1]
    list_off = np.zeros(PROBE_C + 1, np.int32)
    list_off[1:] = np.cumsum([r.size for r in rows])
    rows = np.concatenate(rows)
    cb = util.shape_ivf_tables(d, m, K, IVF_C, IVF_FROM)["codebook"]
    codes = _encode(cb, x[rows] - first[cell[rows]])
    out = dict(coarse=coarse, codebook=cb, list_off=list_off, ids=(rows + 1).astype(np.int32), codes=codes, vectors=x[rows])
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def probe_queries():
    """8 corpus rows; query PROBE_FAR scaled by 10.8: |10.8 q - c|^2 lies between 96 and 139 for unit vectors, below the cell limit
    of 100 only for the few centroids with a cosine above 0.82."""
    qs = np.array(util.shape_queries(6000, 64, 8, seed=5), np.float32)
    qs[PROBE_FAR] *= np.float32(10.8)
    qs.setflags(write=False)
    return qs


@functools.lru_cache(maxsize=None)
def probe_settings():
    """(found rule, sentinel): the reference's; the accepted-rows rule with a sentinel that about 3 rows per query stay under, so
    that most queries go into further rounds, over the cells that are left."""
    t = probe_table()
    return ((0, 1000.0), (1, _inner_sentinel(t, probe_queries()[:PROBE_FAR], 3)))


_probe_dist = []


def probe_distances(oracle):
    """[8][520] the reference's squared distances of the queries to the centroids (the oracle's arithmetic), computed once."""
    if not _probe_dist:
        _probe_dist.append(np.array([[oracle.sqdist(q, c) for c in probe_table()["coarse"]] for q in probe_queries()], np.float32))
    return _probe_dist[0]


def probe_round_one_rows(oracle, ot, W):
    """[8] rows of the lists that the first probing round of each query reads, from the oracle's own cell selection: its
    foundInstances under the reference's rule (rows retrieved) when stopped after one round.  What
    freddy_gpu_last_scanned_rows sums after a call that ended with round one.  It tells which of two equally near cells at the
    W-th place was taken where their lists differ in length -- a choice that follows from updateTopK's arrival order (a
    newcomer is put in front of its equals, so the earlier cell is the first to be pushed out), not from the cell number."""
    _, found, rounds = oracle.ivfadc_search_many(ot, probe_queries(), PROBE_K, W, sentinel=1000.0, found_rule=0, max_rounds=1)
    assert (rounds <= 1).all()
    return found


# ---- D. exact kNN -----------------------------------------------------------------------------------------------------------
EXACT_D = (64, 300)
EXACT_DISTINCT, EXACT_COPIES, EXACT_ORIGINAL = 1000, 2 * 1024 + 3, 7
EXACT_Q = (1, 8, 9, 20)
EXACT_NEG, EXACT_TIE = 3, 6                            # positions of the query equal to minus the copied row, and to the copied row


@functools.lru_cache(maxsize=None)
def exact_table(d):
    """(x, ids): 1000 distinct corpus rows and 2051 copies of row 7 at positions drawn once (3051 rows, ids = 2 row + 3: an even
    number is an unknown id)."""
    N = EXACT_DISTINCT + EXACT_COPIES
    base = util.shape_corpus(EXACT_DISTINCT, d).numpy()
    at = np.sort(np.random.default_rng(17).choice(N, EXACT_COPIES, replace=False))
    x = np.empty((N, d), np.float32)
    x[at] = base[EXACT_ORIGINAL]
    x[np.setdiff1d(np.arange(N), at)] = base
    ids = (np.arange(N) * 2 + 3).astype(np.int32)
    x.setflags(write=False)
    ids.setflags(write=False)
    return x, ids


@functools.lru_cache(maxsize=None)
def exact_queries(d):
    base = util.shape_corpus(EXACT_DISTINCT, d).numpy()
    qs = base[::EXACT_DISTINCT // 20][:20].copy()
    qs[EXACT_TIE] = base[EXACT_ORIGINAL]
    qs[EXACT_NEG] = -qs[EXACT_TIE]
    qs.setflags(write=False)
    return qs


@functools.lru_cache(maxsize=None)
def exact_subsets(d):
    """{"large": 1500 known ids (more rows than every k) + 30 duplicates + 3 unknown ids, "small": 50 known ids (fewer rows than
    every k) + a duplicate + an unknown id, "join": 2000 known ids + 40 duplicates + 2 unknown ids}"""
    _, ids = exact_table(d)
    rng = np.random.default_rng(23)
    big = ids[rng.choice(ids.size, 2000, replace=False)]
    unknown = np.array([4, 10 ** 8, -7], np.int32)
    out = {"large": np.concatenate([big[:1500], big[:30], unknown]), "small": np.concatenate([big[:50], big[:1], unknown[:1]]),
           "join": np.concatenate([big, big[:40], unknown[:2]])}
    return _frozen(out)


# ---- E, F, G. the kNN-join ----------------------------------------------------------------------------------------------------
JOIN_N, JOIN_Q = 6000, 12
JOIN_QUERY_KC = 8


@functools.lru_cache(maxsize=None)
def ivpq_table(kc, dup):
    """An ivpq index of the (64, 8, 16) shape over 6000 rows whose multi-index has kc codewords per half: the halves of kc corpus
    rows drawn per half.  dup: after the rows' cells are fixed, two codewords of each half become bit-for-bit copies of others
    (equal sub-distances for every query: the side sort and the traversal meet equal keys)."""
    d, m, K = SHAPES["0"]
    x = util.shape_corpus(JOIN_N, d).numpy()
    p = util.shape_pq_tables(d, m, K, JOIN_N)
    rng = np.random.default_rng(100 + kc)
    half = d // 2
    # (the corpus repeats 1 % of its rows: codewords are drawn among the rows whose half occurs once, so that equal
    # sub-distances come from `dup` alone)
    once = [np.unique(x[:, h * half:(h + 1) * half], axis=0, return_index=True)[1] for h in range(2)]
    coarse = np.stack([x[np.sort(rng.choice(once[h], kc, replace=False)), h * half:(h + 1) * half] for h in range(2)]).astype(np.float32)
    cell = (_nearest(x[:, :half], coarse[0]) + kc * _nearest(x[:, half:], coarse[1])).astype(np.int32)
    if dup:
        coarse[0, kc - 1], coarse[0, kc // 2] = coarse[0, 1], coarse[0, 0]
        coarse[1, kc - 2], coarse[1, kc // 2 + 1] = coarse[1, 0], coarse[1, 2]
    cells = kc * kc
    stats = np.zeros(cells + 1, np.float32)
    stats[:cells] = np.bincount(cell, minlength=cells).astype(np.float32) / np.float32(JOIN_N)
    stats[cells] = np.float32(JOIN_N)
    out = dict(codebook=p["codebook"], coarse=coarse, ids=p["ids"], coarse_id=cell, codes=p["codes"], vectors=x, stats=stats)
    return _frozen(out)


def ivpq_pin_args(t):
    return (t["codebook"], t["coarse"], t["ids"], t["coarse_id"], t["codes"], t["vectors"], t["stats"])


@functools.lru_cache(maxsize=None)
def join_queries():
    return util.shape_queries(JOIN_N, 64, JOIN_Q, seed=21)


@functools.lru_cache(maxsize=None)
def join_targets():
    """3000 known ids, 30 duplicates, 2 unknown ids"""
    t = np.random.default_rng(31).choice(np.arange(1, JOIN_N + 1), size=3000, replace=False).astype(np.int32)
    t = np.concatenate([t, t[:30], np.array([JOIN_N + 9, -4], np.int32)])
    t.setflags(write=False)
    return t


def join_few_targets():
    """20 known ids: fewer rows than every k of the join's cases"""
    return join_targets()[:20].copy()


JOIN_ALPHA, JOIN_CONF = 3, 0.8


def join_pv_alpha(pvf):
    """alpha of a method 2 call: the first round asks for k alpha expected targets and the selection keeps k pvf of them, so
    alpha = 2 pvf (at least JOIN_ALPHA) makes a round's candidates outnumber the keys kept (asserted with the oracle)."""
    return max(JOIN_ALPHA, 2 * pvf)


JOIN_FEW = dict(k=64, alpha=1, pvf=4)                  # the call over join_few_targets()
SIDE_CALL = dict(k=10, alpha=3, pvf=4)                 # family F: the selection width of the join kernel is not its subject
SIDE_FEW = 129                                         # the coarse_codes whose call is repeated over join_few_targets()


def traverse_small(k, alpha, n_targets, cells):
    """join_run.h launch_traverse: the SMALL kernel (the 64 smallest keys only) is taken when the stop is expected far below 63
    cells, with min_target = k alpha in the first round.  A restatement of a dispatch rule: it breaks when the rule changes."""
    per_cell = n_targets / max(cells, 1)
    return pick_V(cells) > 1 and per_cell > 0.0 and 3.0 * (k * alpha) / per_cell < 31.0


TRAVERSE_DEEP = (10, 250)                              # (k, alpha): 2500 of the 3000 targets expected


def traverse_calls(kc):
    """[(k, alpha)] of one coarse_codes: a call that takes the SMALL kernel (k alpha = 5), one that does not (k = 10 and the
    smallest alpha + 1 at which the predicate fails) and stops within the 64 nearest cells, and the DEEP one, whose stop lies
    beyond 63 cells: only then does the full kernel sort all 64 V keys and walk the chunks behind the first (join_traverse.h).
    64 cells have no SMALL kernel and no second chunk."""
    per_cell = join_targets().size / (kc * kc)
    return [(5, 1), (10, int(31.0 * per_cell / 30.0) + 2), TRAVERSE_DEEP]


def cell_keys(oracle, t, q):
    """[cells] float32: the reference's distance of every cell of the multi-index for the query, 0 + D0[c0] + D1[c1]."""
    kc, half = t["coarse"].shape[1], t["coarse"].shape[2]
    d0 = np.array([oracle.sqdist(q[:half], c) for c in t["coarse"][0]], np.float32)
    d1 = np.array([oracle.sqdist(q[half:], c) for c in t["coarse"][1]], np.float32)
    c = np.arange(kc * kc)
    return (np.float32(0) + d0[c % kc]) + d1[c // kc]


_tie_free = {}


def tie_free_queries(oracle, kc):
    """The queries of join_queries() no two cells of which are equally far in the table ivpq_table(kc, False): the device
    traversal hands a query to the host heap only for equal keys among the cells it takes (or, SMALL, for a stop beyond its
    keys), so these are never handed back for a tie, in any round."""
    if kc not in _tie_free:
        t = ivpq_table(kc, False)
        _tie_free[kc] = [q for q, v in enumerate(join_queries()) if np.unique(cell_keys(oracle, t, v)).size == kc * kc]
    return _tie_free[kc]
