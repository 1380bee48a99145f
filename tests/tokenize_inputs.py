"""The case list of the tokenize tests (tests/test_gpu_tokenize.py; tests/test_tokenize_inputs_cpu.py proves that it can tell
wrong implementations apart): per shape a table of about 2 000 rows with gaps in its ids, and texts of 0, 1, 2, 3, 5, 7, 63, 64,
65, 257 and 4096 ids -- unsorted, with duplicates, with unknown ids mixed in, and of unknown ids only.
  d = 300   75 float4 units: more than one wave of units, not a whole number of waves
  d = 25    the scalar path
  d = 64    16 units: a quarter of a wave
The rows mix magnitudes from 2^-40 to 2^40 inside every column (small terms are absorbed by large sums, so the order of the
additions shows), and hold -0.0 and 0.0."""
import numpy as np

SHAPES = (300, 25, 64)
LENGTHS = (0, 1, 2, 3, 5, 7, 63, 64, 65, 257, 4096)
N_ROWS = 2003


def table(d, seed=11):
    """(ids ascending with gaps, vectors [N][d])"""
    rng = np.random.default_rng(seed + d)
    steps = rng.choice(np.array([1, 1, 1, 2, 5, 40]), size=N_ROWS)
    ids = (7 + np.cumsum(steps)).astype(np.int32)
    v = rng.standard_normal((N_ROWS, d)).astype(np.float32)
    scale = np.exp2(rng.choice(np.array([-40, -10, 0, 0, 0, 10, 40]), size=(N_ROWS, d))).astype(np.float32)
    v = (v * scale).astype(np.float32)
    z = rng.random((N_ROWS, d))
    v[z < 0.01] = np.float32(-0.0)
    v[(z >= 0.01) & (z < 0.02)] = np.float32(0.0)
    v[5] = np.float32(-0.0)   # (a whole row of -0.0)
    return ids, v


def unknown_ids(ids, n, rng):
    """ids no row has: in the gaps, below and above the table, negative, the ends of int32"""
    have = set(int(i) for i in ids)
    gaps = np.array([i for i in range(int(ids[0]), int(ids[-1])) if i not in have], np.int64)
    pool = np.concatenate([gaps, np.array([0, 1, int(ids[0]) - 1, int(ids[-1]) + 1, int(ids[-1]) + 1000, -1, -5, -2 ** 31, 2 ** 31 - 1], np.int64)])
    return rng.choice(pool, size=n).astype(np.int32)


def texts(ids, seed=5):
    """[(name, int32 ids)]: four kinds per length"""
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        if L == 0:
            out.append(("len0", np.empty(0, np.int32)))
            continue
        clean = rng.permutation(ids)[:L] if L <= ids.size else rng.choice(ids, size=L)
        if L >= 2 and np.all(np.diff(clean) > 0):   # (a draw that happens to ascend)
            clean = clean[::-1]
        out.append((f"len{L}_unsorted", np.ascontiguousarray(clean, np.int32)))
        dup = rng.choice(ids[: max(2, min(ids.size, L // 2 + 1))], size=L).astype(np.int32)
        if L >= 2:
            dup[-1] = dup[0]
        out.append((f"len{L}_duplicates", dup))
        mixed = rng.choice(ids, size=L).astype(np.int32)
        bad = rng.random(L) < 0.25
        if L >= 2:
            bad[0], bad[1] = True, False
        mixed[bad] = unknown_ids(ids, int(bad.sum()), rng)
        out.append((f"len{L}_mixed", mixed))
        out.append((f"len{L}_unknown", unknown_ids(ids, L, rng)))
    return out


def ragged(text_list):
    """(token_ids int32, offsets int64[n + 1]) of a list of texts"""
    lens = [len(t) for t in text_list]
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.concatenate(text_list).astype(np.int32) if lens else np.empty(0, np.int32)
    return ids, off
