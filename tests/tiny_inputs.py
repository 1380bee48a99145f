"""The case list of the small-magnitude tests (tests/test_gpu_tiny_magnitudes.py; tests/test_tiny_inputs_cpu.py proves that the
cases are what they claim): one base table of 2 080 x 32 unit-scale rows (65 strips of the exact filter: its threshold comes from a
sample) with gaps in its ids, 70 queries (a pass of 64 and one of 6), and per case the table and / or the queries times a power of
two -- exact in binary32 until the elements themselves leave the normal range.

Cosine similarity is bilinear: a table at 2^-80 searched with unit-scale queries has similarities around 2^-80, normal numbers
that the reference orders strictly, while the SQUARES of its elements (2^-160) are zero in binary32.  A norm taken from a
binary32 sum of squares is then 0 and a bracket scaled by it has no width.

Rows 100 .. 299 are a near-tie cluster: copies of one base row with every element moved by up to 24 ulps (fixed seed).
Query 0 is that row times 4, so its 200 best rows are the cluster, separated by about 1e-7 of their similarity: the rounding of
the reference's chain decides their order, and a filter whose bracket is narrower than that rounding drops true members."""
import functools

import numpy as np

import util

N, D, Q = 2080, 32, 70
CLUSTER = slice(100, 300)
CLUSTER_ROW = 100
MIXED_ROWS = slice(1000, 1100)
SEED = 34
NUDGE_ULPS = 24     # every cluster element moves by -NUDGE_ULPS .. NUDGE_ULPS ulps

# name -> (table exponent, or "mixed": rows MIXED_ROWS x 2^-80 and the rest unit; query exponent;
#          class of the fp32 fma chain of squares over the longest row; the same over query 0)
CASES = {
    "control":                 (-60, 0, "normal", "normal"),
    "squares_subnormal_70":    (-70, 0, "subnormal", "normal"),
    # (unit rows of 32 elements: at 2^-74 a square passes half the smallest subnormal only for an element above 2^-75; the longest
    # row has none and its chain is 0, 209 other rows keep an ulp or two -- the table's MAXIMUM over rows is two ulps, not 0)
    "squares_rounded_away_74": (-74, 0, "zero", "normal"),
    "squares_vanish_80":       (-80, 0, "zero", "normal"),
    "squares_vanish_100":      (-100, 0, "zero", "normal"),
    "tiny_query":              (0, -80, "normal", "zero"),
    "both_small":              (-50, -50, "normal", "normal"),
    # (the exact filter scales both sides to 2^14 and unscales the products by one binary32 power of two: here it is 2^-150 = 0)
    "unscale_underflows":      (-62, -62, "normal", "normal"),
    "elements_subnormal":      (-140, 0, "zero", "normal"),
    "mixed":                   ("mixed", -80, "normal", "zero"),
}
# elements_subnormal: the cluster's similarities for query 0 are one subnormal value, a tie that the ids break
MASSIVE_TIES = ("elements_subnormal",)
# the cases in which the norm of one side vanishes while the similarities stay normal numbers: a bracket of 1e-37 is too narrow
NORM_VANISHES = ("squares_rounded_away_74", "squares_vanish_80", "squares_vanish_100", "tiny_query", "mixed")


@functools.lru_cache(maxsize=None)
def base():
    """(ids int32[N] ascending with gaps, x float32[N][D] with the cluster in it, queries float32[Q][D] with query 0 parallel to it)"""
    x = util.corpus(N, d=D).numpy().astype(np.float32).copy()
    ids = (np.arange(N) * 3 + 2).astype(np.int32)
    rng = np.random.default_rng(SEED)
    row = x[CLUSTER_ROW].copy()
    n = CLUSTER.stop - CLUSTER.start
    nudge = rng.integers(-NUDGE_ULPS, NUDGE_ULPS + 1, size=(n, D)).astype(np.int32)
    x[CLUSTER] = (row.view(np.int32)[None, :] + nudge).view(np.float32)     # (sign-magnitude: +j moves |v| by j ulps)
    qs = rng.standard_normal((Q, D)).astype(np.float32)
    qs[0] = row * np.float32(4.0)
    x.setflags(write=False); ids.setflags(write=False); qs.setflags(write=False)
    return ids, x, qs


@functools.lru_cache(maxsize=None)
def case(name):
    """(ids, table, queries) of a case; read-only arrays, computed once"""
    ids, x, qs = base()
    te, qe = CASES[name][:2]
    if te == "mixed":
        t = x.copy()
        t[MIXED_ROWS] = t[MIXED_ROWS] * np.float32(2.0 ** -80)
    else:
        t = (x * np.float32(2.0 ** te)).astype(np.float32)
    q = (qs * np.float32(2.0 ** qe)).astype(np.float32)
    t.setflags(write=False); q.setflags(write=False)
    return ids, t, q


def scaled_table(exp, d=D, n=N):
    """The first n rows / d columns of the base table times 2^exp (the chains that divide and take square roots: d = 32 and 25)"""
    _, x, _ = base()
    t = np.ascontiguousarray(x[:n, :d] * np.float32(2.0 ** exp), dtype=np.float32)
    return t


def fma_chain_of_squares(v):
    """n2 = fmaf(v_i, v_i, n2) in binary32, i ascending: the product is exact in binary64, the sum rounded once to binary32"""
    n2 = np.float32(0.0)
    for e in np.asarray(v, np.float32):
        n2 = np.float32(np.float64(e) * np.float64(e) + np.float64(n2))
    return n2


def classify(v):
    v = abs(float(v))
    if v == 0.0:
        return "zero"
    return "subnormal" if v < 2.0 ** -126 else "normal"
