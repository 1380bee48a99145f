"""The cases of tests/exact_ids_inputs.py reach what they claim (no GPU): the restatements agree with a plain loop, and the tables
and id sets of tests/test_gpu_resolve.py put rows where the device resolve (csrc/resolve.h) changes its path -- the last, partly
filled bitmap word, tables smaller than one word, the first and the last word, more than one block, a block of several 64-word
steps, both sides of a chunk boundary of the shared scan, and grids smaller than their work under option grid_cus = 1."""
import os
import re

import numpy as np
import pytest

import exact_ids_inputs as ei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows_slow(table, ids):
    pos = {int(v): r for r, v in enumerate(table)}
    return np.array(sorted({pos[int(i)] for i in ids if int(i) in pos}), np.int32)


@pytest.mark.parametrize("style", ["gaps", "serial"])
@pytest.mark.parametrize("N", [1, 31, 33, 700])
def test_rows_of_ids_restatement_equals_a_plain_loop(N, style):
    table = ei.table_ids(N, style)
    for name, s in ei.id_sets(table, seed=N).items():
        got = ei.rows_of_ids(table, s)
        assert np.array_equal(got, _rows_slow(table, s)), name
        assert np.all(np.diff(got) > 0), name
    assert ei.rows_of_ids(table, ei.id_sets(table)["unknown"]).size == 0
    assert ei.rows_of_ids(table, ei.id_sets(table)["thrice"]).size == N


def test_id_rule_restatement():
    table = ei.table_ids(50, "gaps")
    q = np.array([table[7], 5, table[3], table[7], -1], np.int32)
    sel, rows = ei.select(table, q, ei.TABLE_ORDER)
    assert sel.tolist() == [table[3], table[7]] and rows.tolist() == [3, 7]
    sel, rows = ei.select(table, q, ei.POSITIONAL)
    assert sel.tolist() == q.tolist() and rows.tolist() == [7, -1, 3, 7, -1]


def test_constants_are_those_of_the_sources():
    src = open(os.path.join(ROOT, "postgres-word2vec_amd", "csrc", "resolve.h")).read()
    sim = open(os.path.join(ROOT, "postgres-word2vec_amd", "csrc", "similarity.h")).read()
    assert int(re.search(r"RESOLVE_BLOCK = (\d+);", src).group(1)) == ei.DEFAULT_BLOCK
    assert int(re.search(r"SIM_CHUNK = (\d+);", sim).group(1)) == ei.SCAN_CHUNK
    assert "b / SIM_CHUNK" in src and "ws += 64" in src


def test_tables_cover_the_word_boundaries():
    Ns = sorted({N for N, _ in ei.RESOLVE_CASES})
    assert any(N < 32 for N in Ns) and 1 in Ns               # tables inside one word
    assert 32 in Ns and 33 in Ns                             # exactly one word, and one row into the second
    assert any(N % 32 != 0 and N > 64 for N in Ns)           # a ragged last word behind full ones
    assert {b for N, b in ei.RESOLVE_CASES if N == 9001} >= {0, 8}


@pytest.mark.parametrize("N,block", ei.RESOLVE_CASES)
def test_sets_reach_first_and_last_word_and_every_block(N, block):
    words, blocks, chunks, B = ei.geometry(N, block)
    table = ei.table_ids(N, "gaps")
    sets = ei.id_sets(table, seed=N)
    every = ei.rows_of_ids(table, sets["every"])
    assert every.size == N and set(ei.word_of(every).tolist()) == set(range(words))
    ends = ei.rows_of_ids(table, sets["ends"])
    assert ei.word_of(ends).min() == 0 and ei.word_of(ends).max() == words - 1
    assert sets["thrice"].size == 3 * N and (N == 1 or sets["thrice"].size > N)       # n > N
    assert set(ei.block_of(every, block).tolist()) == set(range(blocks))
    tenth = ei.rows_of_ids(table, sets["tenth"])
    assert 0 < tenth.size < sets["tenth"].size                                       # duplicates and unknown ids were mixed in
    if blocks > 1:
        assert len(set(ei.block_of(tenth, block).tolist())) >= 2                      # rows in two different blocks
        assert (np.bincount(ei.block_of(tenth, block), minlength=blocks) == 0).any() or blocks <= 40   # (and, in large tables, blocks without a row)


def test_blocks_steps_and_chunks():
    g = {c: ei.geometry(*c) for c in ei.RESOLVE_CASES}
    assert g[(9001, 8)][:3] == (282, 36, 1) and g[(9001, 0)][:3] == (282, 2, 1)
    # a block of more than one step of 64 words, with a ragged last step, and a ragged last block
    words, blocks, chunks, B = g[(9001, 200)]
    assert B > ei.WAVE_WORDS and B % ei.WAVE_WORDS != 0 and blocks == 2 and words % B != 0
    # the second level of the scan: only the 40 000-row table at one word per block has blocks in two chunks
    assert [c for c in ei.RESOLVE_CASES if g[c][2] > 1] == [(40000, 1)]
    words, blocks, chunks, B = g[(40000, 1)]
    assert (blocks, chunks) == (1250, 2)
    table = ei.table_ids(40000, "gaps")
    for name in ("every", "thrice", "tenth"):
        rows = ei.rows_of_ids(table, ei.id_sets(table, seed=40000)[name])
        ch = ei.chunk_of(rows, 1)
        assert set(ch.tolist()) == {0, 1}, name
        boundary = ei.SCAN_CHUNK * B * 32
        assert (rows < boundary).any() and (rows >= boundary).any(), name
    every = ei.rows_of_ids(table, table)
    assert {boundary - 1, boundary} <= set(every.tolist())


def test_grid_cus_1_makes_every_loop_go_round():
    wgs = 1 * ei.GRID_WGS_PER_CU
    for N, block in ((9001, 8), (40000, 1)):
        words, blocks, _, _ = ei.geometry(N, block)
        assert 3 * N > 2 * wgs * 256          # the mark kernel: every lane takes more than two ids of the tripled set
        assert blocks > wgs * 4               # count / place: more blocks than waves
