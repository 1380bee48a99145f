"""tests/statistics_model.py, the numpy model the GPU tests of create_statistics compare with, against a plain Python loop
written from the SQL (freddy--0.0.1.sql:150-171), and the one case that tells a float64 division from a float32 one."""
import struct

import numpy as np
import pytest

import statistics_model as sm


def _sql(table_ids, table_cell, cells, column):
    """create_statistics as the SQL states it: total over the join of the column with the table, then one count per cell"""
    cell_of = {int(i): int(c) for i, c in zip(table_ids, table_cell)}
    column = list(table_ids) if column is None else [int(i) for i in column]
    total = sum(1 for i in column if i in cell_of)                       # count(*) ... INNER JOIN
    if total == 0:
        raise ZeroDivisionError
    out = []
    for c in range(cells):
        n = sum(1 for i in column if cell_of.get(i) == c)
        out.append(struct.unpack("f", struct.pack("f", n / total))[0])   # float8 division, stored as float4
    out.append(struct.unpack("f", struct.pack("f", float(total)))[0])
    return np.array(out, np.float32), total


def _table(n=500, cells=9, gaps=True, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(1, 4 * n), n, replace=False)) if gaps else np.arange(1, n + 1)
    return ids.astype(np.int32), rng.integers(0, cells, n).astype(np.int32), cells


@pytest.mark.parametrize("gaps", [False, True])
def test_model_equals_the_sql_loop(gaps):
    ids, cell, cells = _table(gaps=gaps)
    rng = np.random.default_rng(1)
    for column in (None, ids[rng.integers(0, ids.size, 700)], ids[:1], ids[cell == 3]):
        got, matched = sm.create_statistics(ids, cell, cells, column)
        exp, total = _sql(ids, cell, cells, column)
        assert matched == total and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_multiplicity_and_unknown_ids():
    ids, cell, cells = _table()
    column = np.concatenate([np.repeat(ids[7], 5), ids[10:20], [0, -4, int(ids[-1]) + 1, 2 ** 31 - 1], np.setdiff1d(np.arange(1, 40), ids)[:3]])
    got, matched = sm.create_statistics(ids, cell, cells, column)
    exp, total = _sql(ids, cell, cells, column)
    assert matched == total == 15
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    count, _ = sm.counts(ids, cell, cells, column)
    assert count[cell[7]] >= 5, "an id listed five times counts five times"
    once, m1 = sm.create_statistics(ids, cell, cells, np.unique(column))
    assert m1 == 11 and not np.array_equal(once, got)


def test_zero_total_raises():
    ids, cell, cells = _table()
    with pytest.raises(sm.ZeroTotal):
        sm.create_statistics(ids, cell, cells, np.array([0, -1, int(ids[-1]) + 7]))
    with pytest.raises(sm.ZeroTotal):
        sm.create_statistics(ids, cell, cells, np.zeros(0, np.int32))
    with pytest.raises(sm.ZeroTotal):
        sm.create_statistics(ids[:0], cell[:0], cells)


def test_a_count_above_2_pow_24_tells_float64_division_from_float32():
    """float32(count) / float32(total) rounds the operands first; the reference divides in float8.  The two agree for all
    integers below 2^24 (both operands exact, and rounding a binary64 quotient to binary32 is innocuous), so only a count above
    2^24 tells the implementations apart: count = 2^24 + 3 of total = 40 000 001."""
    count, total = 2 ** 24 + 3, 40_000_001
    assert float(np.float32(count)) != count and float(np.float32(total)) != total
    got = sm.row_from_counts([count, total - count], total)
    wrong = np.float32(count) / np.float32(total)
    assert got[0].view(np.uint32) != wrong.view(np.uint32), "the case does not bite"
    assert got[0] == np.float32(count / total) and got[2] == np.float32(total) and float(got[2]) == 40_000_000.0
    small = np.arange(1, 2000)
    assert np.array_equal((small.astype(np.float64) / 1999.0).astype(np.float32), small.astype(np.float32) / np.float32(1999))
