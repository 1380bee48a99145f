"""The inputs of the statistics swap (tests/statistics_inputs.py) on the CPU oracle alone: rows A and B make the kNN-join take
different numbers of cells and answer with different lists, so a GPU test that swaps A for B cannot pass on a library that
ignores the call or updates only one copy of the row."""
import numpy as np

import statistics_inputs as si


def test_rows_a_and_b_differ_and_are_well_formed():
    a, b = si.row_a(), si.row_b()
    cells = si.cells()
    assert a.dtype == b.dtype == np.float32 and a.size == b.size == cells + 1
    assert a[cells] == si.N and b[cells] == si.column().size - 2          # (two ids of the column have no row)
    assert np.array_equal(a.view(np.uint32), si.tables()["stats"].view(np.uint32)), "A is the row the index build computes"
    assert np.sort(b[:cells])[-4:].sum() > 0.9 > np.sort(a[:cells])[-4:].sum(), "B is concentrated in four cells, A is not"
    assert si.targets().size < si.column().size - 2, "the column has duplicates"


def test_the_swap_changes_cell_counts_iterations_and_lists(oracle):
    ta, tb = si.oracle_table(oracle, "A"), si.oracle_table(oracle, "B")
    qs, targets = si.queries(), si.targets()
    for k, alpha in si.CALLS:
        ca, _ = oracle.multi_index_select(ta, qs, np.arange(si.Q), targets.size, k * alpha, si.CONFIDENCE)
        cb, _ = oracle.multi_index_select(tb, qs, np.arange(si.Q), targets.size, k * alpha, si.CONFIDENCE)
        na, nb = np.array([c.size for c in ca]), np.array([c.size for c in cb])
        assert (na != nb).sum() >= si.Q // 2, (k, alpha, na.tolist(), nb.tolist())
        for method in si.METHODS:
            (ea, ia), (eb, ib) = si.expected(oracle, "A", method, k, alpha), si.expected(oracle, "B", method, k, alpha)
            assert ia != ib, (k, alpha, method, ia, ib)
            assert (ea["id"] != eb["id"]).any(axis=1).sum() >= 1, (k, alpha, method)
