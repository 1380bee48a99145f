"""The case tables of the similarity tests (tests/test_gpu_similarity.py); tests/test_similarity_inputs_cpu.py proves on the CPU that
they reach what they are meant to reach."""
import functools

import numpy as np

import util

DIMS = (300, 25, 32, 7)          # 16-byte loads with a last chunk of 12 dimensions; scalar loads, d < 32 and d odd; one exact chunk
PAIR_N = (0, 1, 63, 64, 65, 130)
MATRIX_NA = (1, 15, 16, 17, 33)
MATRIX_NB = (1, 63, 64, 65, 200)
TABLE_ROWS = 3000


@functools.lru_cache(maxsize=None)
def table(d, n=TABLE_ROWS):
    """(ids[n] ascending with gaps, x[n][d] float32) -- rows of util.shape_corpus (1 % of them copies of other rows)"""
    x = util.shape_corpus(n, d).numpy().astype(np.float32)
    rng = np.random.default_rng(50 + d)
    ids = (10 + np.cumsum(rng.integers(1, 4, size=n))).astype(np.int32)      # first id >= 11, gaps of 0 .. 2 ids between neighbours
    return ids, x


def unknown_ids(ids):
    """ids without a row: below the first, above the last, and in the gaps"""
    ids = np.asarray(ids, np.int64)
    gaps = np.setdiff1d(np.arange(ids[0], ids[-1]), ids)
    return np.concatenate([[ids[0] - 7, ids[0] - 1, ids[-1] + 1, ids[-1] + 1000], gaps[:: max(1, gaps.size // 8)][:8]]).astype(np.int32)


def draw_ids(ids, n, rng, unknown=True):
    """n ids of the table in any order with repeats; about one in six replaced by an id without a row"""
    out = ids[rng.integers(0, ids.size, size=n)].copy()
    if n >= 3:
        out[n // 2] = out[0]                                                  # the same id twice within a side
    if unknown and n:
        bad = unknown_ids(ids)
        at = rng.random(n) < 1 / 6
        out[at] = bad[rng.integers(0, bad.size, size=int(at.sum()))]
    return out.astype(np.int32)


def pair_case(d, n, seed=0):
    ids, _ = table(d)
    rng = np.random.default_rng(1000 * d + n + seed)
    a, b = draw_ids(ids, n, rng), draw_ids(ids, n, rng)
    if n >= 2:
        b[1] = a[1] = ids[5]                                                  # the same id on both sides
    if n >= 65:
        a[3], b[64] = ids[0] - 1, ids[-1] + 1                                 # below the first, above the last
    return a, b


def matrix_case(d, na, nb, seed=0):
    ids, _ = table(d)
    rng = np.random.default_rng(77 * d + 1000 * na + nb + seed)
    a, b = draw_ids(ids, na, rng, unknown=na > 1), draw_ids(ids, nb, rng, unknown=nb > 1)
    if na >= 15 and nb >= 63:
        a[2], b[7] = ids[9], ids[9]                                           # the same id on both sides
        a[5], b[11] = ids[0] - 1, ids[-1] + 1
    return a, b


def join_threshold(out, ka, kb, frac=0.1):
    """a threshold that passes about `frac` of the known pairs: a value of the matrix itself, so equality occurs"""
    v = out[np.ix_(ka, kb)].ravel()
    v = np.sort(v[~np.isnan(v)])
    return np.float32(v[int((1 - frac) * (v.size - 1))]) if v.size else np.float32(0.0)


# ---- the constructed join: rows with a few non-zero small coordinates whose chains are exact -------------------------------------
THR = np.float32(0.75)
THR_UP = np.nextafter(THR, np.float32(1.0))          # one ulp above
CON_NB = 200                                          # three full 64-blocks and one of 8 lanes


def constructed(d):
    """-> (ids, x, a_ids, b_ids, thresholds).  Every A row is c * e0, so its similarity to B row j is c * x[j][0] exactly (the other
    products are +-0): with c = 2 and x[j][0] = s[j] / 2 the row of similarities is s, chosen per lane:
        block 0 (j 0 .. 63)      0.25 everywhere                                  no match
        block 1 (j 64 .. 127)    0.25, lane 63 = THR_UP                            one match, in the last lane
        block 2 (j 128 .. 191)   1.0 everywhere                                    64 matches, lane 0 right behind j = 127
        block 3 (j 192 .. 199)   THR (equal: no match), THR_UP, NaN, -THR_UP, then 0.25; j = 197 is an id without a row
    A rows: 2 e0 (the pattern), -2 e0 (its negative: the NaN and j = 195 match), the zero row (+0.0 everywhere, NaN at the NaN: against the
    threshold -0.0 nothing but the NaN matches), an id without a row, and 2 e0 again (a repeated id)."""
    s = np.full(CON_NB, 0.25, np.float32)
    s[127] = THR_UP
    s[128:192] = 1.0
    s[192:196] = [THR, THR_UP, np.nan, -THR_UP]
    n = CON_NB + 3
    x = np.zeros((n, d), np.float32)
    x[:CON_NB, 0] = s / np.float32(2.0)
    x[:CON_NB, d - 1] = 3.0                            # (a coordinate the A rows do not have: its products are zeros)
    x[CON_NB, 0], x[CON_NB + 1, 0] = 2.0, -2.0         # row CON_NB + 2 stays zero
    ids = (100 + 2 * np.arange(n)).astype(np.int32)
    b_ids = ids[:CON_NB].copy()
    b_ids[197] = 101
    a_ids = np.array([ids[CON_NB], ids[CON_NB + 1], ids[CON_NB + 2], 7, ids[CON_NB]], np.int32)
    return ids, x, a_ids, b_ids, (THR, np.float32(-0.0), np.float32(np.nan), np.float32(-np.inf), np.float32(np.inf))


# ---- the soak: a dozen drawn shapes ----------------------------------------------------------------------------------------------
def soak_cases(n=12, seed=2024):
    """(d, na, nb, n_pairs, by_vectors, frac) -- d % 4 both ways, up to a few hundred per side"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        d = int(rng.choice([300, 32, 64, 100] if i % 2 == 0 else [25, 7, 35, 301]))
        out.append((d, int(rng.integers(1, 300)), int(rng.integers(1, 400)), int(rng.integers(1, 500)), bool(i % 3 == 0), float(rng.choice([0.0, 0.01, 0.3]))))
    return out


# ---- non-finite rows among healthy ones ------------------------------------------------------------------------------------------
def poisoned_table(d):
    """(ids, x, poisoned row numbers): table(d) with inf, NaN and values whose products overflow in eight rows"""
    ids, x = table(d)
    x = x.copy()
    rows = np.array([3, 64, 65, 700, 701, 1500, 2998, 2999])
    x[3, 0] = np.inf
    x[64, d - 1] = -np.inf
    x[65, d // 2] = np.nan
    x[700, :] = np.nan
    x[701, 0], x[701, d - 1] = np.inf, -np.inf
    x[1500, 1] = 3e38
    x[2998, 1] = -3e38                                 # (the pair 1500 x 2998 overflows to -inf in its second product)
    x[2999, 0] = util.NEG_NAN
    return ids, x, rows
