"""The threshold rank, as a property of the reference's insertion loop -- pure Python, no GPU.

The filter + refine kernels cut on a CHEAP bound and run the reference's arithmetic only for the rows the cut lets through.  The cut
is taken at the k-th smallest cheap bound (W-th for the cell choice), not at the 2k-th: 2k is the number of exact KEYS that
selection-then-replay keeps, k is enough as the RANK of a threshold.  With the bracket d_lo <= d <= d_lo + E and t >= the k-th
smallest d_lo, the set S = {d_lo <= t + E} holds every row at or below the k-th smallest exact distance, ties included, and

    replay(S in scan order)  ==  replay(the 2k smallest (distance, position) keys of S, in scan order)  ==  replay(everything).

The streams carry heavy ties, carried lists with fewer than k real entries, rows at the sentinel and NaN rows; all values are
multiples of 1/4, so the brackets hold exactly in binary32."""
import numpy as np

from test_oracle import py_stream

f32 = np.float32
INF = f32(np.inf)


def kth_smallest(values, k):
    """the k-th smallest of the non-NaN values, +inf if there are fewer than k (the kernels then keep every row)"""
    v = np.sort(np.asarray(values, f32)[~np.isnan(values)])
    return v[k - 1] if len(v) >= k else INF


def lane_minima(values, rng, lanes):
    """what the kernels really sort: the minima of `lanes` disjoint groups of the values (NaNs never enter a minimum)"""
    group = rng.integers(0, lanes, size=len(values))
    out = []
    for g in range(lanes):
        v = np.asarray(values, f32)[group == g]
        v = v[~np.isnan(v)]
        if len(v):
            out.append(v.min())
    return np.asarray(out, f32)


def keys_2k(d, pos, keep, k2):
    """the k2 smallest (distance bits, position) keys among the rows `keep`, back in scan order"""
    keep = np.asarray(keep, np.int64)
    order = np.lexsort((pos[keep], d[keep].view(np.uint32)))[:k2]
    return np.sort(keep[order])


def test_rows_cut_at_the_kth_smallest_bound():
    rng = np.random.default_rng(20)
    sentinel = f32(100.0)
    for trial in range(6000):
        k = int(rng.integers(1, 11))
        n = int(rng.integers(0, 140))
        levels = int(rng.integers(1, 10))
        E = f32((0.25, 0.5, 1.0)[trial % 3])
        d = (rng.integers(0, levels, size=n) / 4 + 2).astype(f32)
        if trial % 5 == 0 and n:
            d[rng.integers(0, n, size=3)] = sentinel                      # rows the guard rejects
        if trial % 7 == 0 and n:
            d[rng.integers(0, n, size=2)] = f32(np.nan)
        # the cheap bound: d_lo <= d <= d_lo + E, at both ends of the bracket and in between
        u = rng.integers(0, 5, size=n) / 4
        if trial % 4 == 1:
            u[:] = 0.0
        if trial % 4 == 2:
            u[:] = 1.0
        lo = (d - u * E).astype(f32)
        assert np.all((lo <= d) & (d <= lo + E) | np.isnan(d))
        pos = np.sort(rng.permutation(2000)[:n])
        carried = None
        if trial % 2 == 0:
            c = int(rng.integers(0, k))                                    # fewer than k real entries
            cd = (rng.integers(0, levels, size=c) / 4 + 2).astype(f32)
            carried = py_stream(cd, -2 - np.arange(c), k, sentinel)
        full = py_stream(d, pos, k, sentinel, carried)
        # the cut: the k-th smallest bound itself, or the k-th smallest of lane minima (never smaller)
        t = kth_smallest(lo, k)
        if trial % 3 == 1:
            t_lanes = kth_smallest(lane_minima(lo, rng, 64), k)
            assert t_lanes >= t
            t = t_lanes
        S = np.flatnonzero((lo <= t + E) | np.isnan(lo))                  # (NaN rows pass every threshold)
        assert py_stream(d[S], pos[S], k, sentinel, carried) == full, (trial, k, "S")
        K2 = keys_2k(d, pos, S, 2 * k)
        assert py_stream(d[K2], pos[K2], k, sentinel, carried) == full, (trial, k, "2k keys of S")


def test_rows_cut_per_chunk_then_per_query():
    """The scan cuts every (item, chunk) at ITS k-th smallest lane minimum + E, the merge cuts the survivors of all chunks at
    their k-th smallest bound + E: two nested cuts, the same list."""
    rng = np.random.default_rng(21)
    sentinel = f32(100.0)
    for trial in range(1500):
        k = int(rng.integers(1, 8))
        n = int(rng.integers(0, 160))
        levels = int(rng.integers(1, 8))
        E = f32(0.5)
        d = (rng.integers(0, levels, size=n) / 4 + 2).astype(f32)
        if trial % 6 == 0 and n:
            d[rng.integers(0, n)] = f32(np.nan)
        lo = (d - rng.integers(0, 3, size=n) / 4).astype(f32)
        pos = np.arange(n)
        chunk = np.sort(rng.integers(0, 4, size=n))
        full = py_stream(d, pos, k, sentinel)
        surv = []
        for c in range(4):
            rows = np.flatnonzero(chunk == c)
            t = kth_smallest(lane_minima(lo[rows], rng, 8), k)
            surv.extend(rows[(lo[rows] <= t + E) | np.isnan(lo[rows])])
        surv = np.asarray(surv, np.int64)
        T = kth_smallest(lo[surv], k)
        S = surv[(lo[surv] <= T + E) | np.isnan(lo[surv])]
        K2 = keys_2k(d, pos, S, 2 * k)
        assert py_stream(d[K2], pos[K2], k, sentinel) == full, (trial, k)


def test_cells_cut_at_the_wth_smallest_approximate_distance():
    """The cell choice: |a - d| <= eps, candidates = {a <= tau + 2 eps} with tau >= the W-th smallest a, a guard limit in place of
    the sentinel, cells offered in ascending id."""
    rng = np.random.default_rng(22)
    for trial in range(3000):
        W = int(rng.integers(1, 12))
        C = int(rng.integers(1, 90))
        levels = int(rng.integers(1, 8))
        eps = f32((0.25, 0.5)[trial % 2])
        d = (rng.integers(0, levels, size=C) / 4 + 3).astype(f32)
        limit = f32(100.0) if trial % 3 else f32(3 + rng.integers(0, levels + 1) / 4)   # a guard inside the data
        if trial % 7 == 0:
            d[rng.integers(0, C)] = f32(np.nan)
        a = (d + rng.integers(-1, 2, size=C) * eps).astype(f32)
        cells = np.arange(C)
        full = py_stream(d, cells, W, limit)
        tau = kth_smallest(a, W)
        if trial % 2:
            tau = kth_smallest(lane_minima(a, rng, 16), W)                # lane or tile minima
        S = np.flatnonzero((a <= tau + 2 * eps) | np.isnan(a))
        assert py_stream(d[S], cells[S], W, limit) == full, (trial, W, "candidates")
        K2 = keys_2k(d, cells, S, 2 * W)
        assert py_stream(d[K2], cells[K2], W, limit) == full, (trial, W, "2W keys of the candidates")
        # the plan's shortcut (<= 64 candidates): without a tie among the W + 1 smallest candidates the list is the W smallest
        # below the limit, ascending
        Sf = S[~np.isnan(d[S])]
        order = Sf[np.lexsort((cells[Sf], d[Sf].view(np.uint32)))]
        top = d[order[:W + 1]]
        if len(np.unique(top)) == len(top):
            short = [(int(c), d[c]) for c in order[:W] if d[c] < limit]
            short += [(-1, limit)] * (W - len(short))
            assert short == full, (trial, W, "shortcut")
