"""Inputs of tests/test_gpu_resolve.py and tests/test_gpu_exact_ids.py, and numpy restatements of what they are compared with:
the id rule of the *_ids calls (include/freddy_gpu.h) and rows_of_ids (csrc/internal.h).  tests/test_exact_ids_inputs_cpu.py
proves on the CPU that the cases reach what they claim (words, blocks and chunks of the device resolve, csrc/resolve.h)."""
import numpy as np

TABLE_ORDER, POSITIONAL = 0, 1

# ---- csrc/resolve.h in numbers --------------------------------------------------------------------------------------------------
DEFAULT_BLOCK = 256     # RESOLVE_BLOCK: bitmap words per block when option resolve_block is 0
SCAN_CHUNK = 1024       # SIM_CHUNK: blocks per chunk of the shared scan (the second level)
WAVE_WORDS = 64         # words one wave takes per step of a block
GRID_WGS_PER_CU = 8     # workgroups per CU the resolve's grids are capped at; 256 ids per workgroup of the mark kernel, 4 blocks
                        # (one per wave) per workgroup of the count and place kernels


def geometry(N, block):
    """(words, blocks, chunks, words per block) of a table of N rows under option resolve_block = block"""
    B = block if block > 0 else DEFAULT_BLOCK
    words = (N + 31) // 32
    blocks = (words + B - 1) // B
    return words, blocks, (blocks + SCAN_CHUNK - 1) // SCAN_CHUNK, B


def word_of(rows):
    return np.asarray(rows) >> 5


def block_of(rows, block):
    return word_of(rows) // (block if block > 0 else DEFAULT_BLOCK)


def chunk_of(rows, block):
    return block_of(rows, block) // SCAN_CHUNK


# (N, resolve_block): the issue's sizes at the default (256 words: four 64-word steps) and at 8 words; 200 words (the last step of a
# block ragged); and one table of 40 000 rows at 1 word per block -- 1 250 blocks, the only case
# with a second chunk of the scan: at 9 001 rows and 8 words there are 36 blocks, all in chunk 0
RESOLVE_CASES = [(N, b) for N in (1, 31, 32, 33, 9001) for b in (0, 8)] + [(9001, 200), (40000, 1)]


def table_ids(N, style):
    """'gaps': 3 r + 1 (no id is its own row: the binary search); 'serial': r + 1 (the first probe hits)"""
    r = np.arange(N, dtype=np.int64)
    return (3 * r + 1 if style == "gaps" else r + 1).astype(np.int32)


def id_sets(ids, seed=0):
    """name -> the id sets of the issue for a table with these ascending ids"""
    rng = np.random.default_rng(seed)
    N = ids.size
    lo, hi = int(ids[0]), int(ids[-1])
    gap = [g for g in (int(ids[N // 2]) + 1,) if g < hi and g not in set(ids.tolist())]   # between two ids, where the table has gaps
    unknown = np.array([lo - 1, lo - 1000, hi + 1, hi + 10**6, -5, 2**31 - 1, -2**31] + gap, np.int32)
    tenth = ids[rng.choice(N, max(N // 10, 1), replace=False)]
    mixed = np.concatenate([tenth, tenth[: max(tenth.size // 3, 1)], unknown, unknown[:2]])
    return {
        "empty": np.zeros(0, np.int32),
        "one": ids[N // 3:N // 3 + 1].copy(),
        "unknown": unknown,
        "every": ids.copy(),
        "thrice": rng.permutation(np.concatenate([ids, ids, ids])).astype(np.int32),
        "tenth": rng.permutation(mixed).astype(np.int32),
        "ends": np.array([ids[-1], ids[0], ids[-1]], np.int32),
    }


# ---- restatements ---------------------------------------------------------------------------------------------------------------
def rows_of_ids(table, ids):
    """rows_of_ids: the table rows of the ids that have one, ascending and distinct"""
    table, ids = np.asarray(table, np.int64), np.asarray(ids, np.int64).reshape(-1)
    if table.size == 0 or ids.size == 0:
        return np.zeros(0, np.int32)
    p = np.searchsorted(table, ids)
    ok = (p < table.size) & (table[np.minimum(p, table.size - 1)] == ids)
    return np.unique(p[ok]).astype(np.int32)


def select(table, query_ids, rule):
    """The id rule: (sel[Q] the selected ids, rows[Q] their table rows or -1)"""
    q = np.asarray(query_ids, np.int32).reshape(-1)
    if rule == TABLE_ORDER:
        rows = rows_of_ids(table, q)
        return np.asarray(table)[rows].astype(np.int32), rows
    t = np.asarray(table, np.int64)
    p = np.searchsorted(t, q.astype(np.int64))
    ok = (p < t.size) & (t[np.minimum(p, max(t.size - 1, 0))] == q) if t.size else np.zeros(q.size, bool)
    return q.copy(), np.where(ok, p, -1).astype(np.int32)


# ---- the join / search cases of tests/test_gpu_exact_ids.py -----------------------------------------------------------------------
JOIN_N, JOIN_D, JOIN_KNOWN = 20000, 300, 9000   # filter + refine: >= 8000 known rows in the set
JOIN_Q = (1, 33, 65, 129)                       # one query (read in place), and tails of the 32-, 64- and 128-query tiles


def join_targets(ids, n_known, seed=2):
    """n_known distinct known ids, 60 of them twice, unknown ids below, above and between; shuffled"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(ids.size, n_known, replace=False)
    t = np.concatenate([ids[rows], ids[rows[:60]], np.array([-7, 10**8], np.int32), (ids[:37].astype(np.int64) + 1).astype(np.int32)])
    return rng.permutation(t).astype(np.int32)


def query_ids(ids, Q, seed):
    """Q distinct known ids, in an order that is not the table's"""
    rng = np.random.default_rng(seed)
    return ids[rng.choice(ids.size, Q, replace=False)].astype(np.int32)
