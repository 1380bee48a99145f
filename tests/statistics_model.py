"""Numpy model of freddy_gpu_create_statistics (include/freddy_gpu.h): create_statistics() of the reference
(freddy--0.0.1.sql:150-171) over the rows of an ivpq table.

    count[c] = entries of the column whose row lies in cell c     (an id listed r times counts r times: the SQL is an INNER JOIN)
    total    = entries that have a row                            (an id no row has is skipped)
    stats[c]     = float32(float64(count[c]) / float64(total))    "count(*)::float / total_amount": float8, stored as float4
    stats[cells] = float32(total)                                 bigint -> float4, round to nearest even

total == 0 is the SQL's division by zero: ZeroTotal."""
import numpy as np


class ZeroTotal(ZeroDivisionError):
    pass


def row_from_counts(count, total):
    """The row of given integer counts (any integers, also beyond what an array could hold entries for)."""
    if total == 0:
        raise ZeroTotal("no entry of the column has a row")
    stats = np.empty(len(count) + 1, np.float32)
    stats[:-1] = (np.asarray(count, np.float64) / np.float64(total)).astype(np.float32)
    stats[-1] = np.float32(total)
    return stats


def counts(table_ids, table_cell, cells, ids=None):
    """(count[cells] as int64, total) of the column `ids` (None: every row of the table once) over a table with ascending ids."""
    table_ids = np.asarray(table_ids, np.int64)
    table_cell = np.asarray(table_cell, np.int64)
    if ids is None:
        hit_cell = table_cell
    else:
        ids = np.asarray(ids, np.int64).reshape(-1)
        at = np.searchsorted(table_ids, ids)
        at[at == table_ids.size] = 0
        known = table_ids[at] == ids if table_ids.size else np.zeros(ids.size, bool)
        hit_cell = table_cell[at[known]]
    count = np.bincount(hit_cell, minlength=cells).astype(np.int64)
    return count, int(count.sum())


def create_statistics(table_ids, table_cell, cells, ids=None):
    """-> (stats [cells + 1] float32, matched)"""
    count, total = counts(table_ids, table_cell, cells, ids)
    return row_from_counts(count, total), total
