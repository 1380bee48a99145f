"""-m gpu: the device resolve alone (csrc/resolve.h) through freddy_gpu_debug_resolve_ids: an id set becomes the ascending, distinct
table rows of its known ids -- compared, as equal arrays, with the numpy restatement of rows_of_ids (tests/exact_ids_inputs.py, which
tests/test_exact_ids_inputs_cpu.py holds to a plain loop and whose cases it proves to reach every word, block and chunk boundary)."""
import numpy as np
import pytest

import exact_ids_inputs as ei

pytestmark = pytest.mark.gpu

D = 16
RESOLVE_KERNELS = {"resolve_mark", "resolve_scan", "resolve_place"}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _vectors(N, seed=0):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)


def _check_sets(idx, table, seed, what):
    for name, s in ei.id_sets(table, seed=seed).items():
        got = idx.debug_resolve_ids(s)
        exp = ei.rows_of_ids(table, s)
        assert got.dtype == np.int32 and np.array_equal(got, exp), (what, name, got[:8].tolist(), exp[:8].tolist(), got.size, exp.size)


@pytest.mark.parametrize("style", ["gaps", "serial"])
@pytest.mark.parametrize("N,block", ei.RESOLVE_CASES)
def test_resolve_equals_rows_of_ids(gpu, N, block, style):
    """Every table size and block size of the case list, ids 3 r + 1 (binary search) and r + 1 (the first probe hits); then the same
    with every grid planned for ONE CU, where the kernels' loops go round more than once."""
    table = ei.table_ids(N, style)
    idx = gpu.VectorIndex(table, _vectors(N))
    idx.set_option("resolve_block", block)
    _check_sets(idx, table, N, f"N={N} block={block} {style}")
    idx.set_option("grid_cus", 1)
    _check_sets(idx, table, N + 1, f"N={N} block={block} {style} grid_cus=1")
    idx.close()


def test_profile_names_the_three_stages_and_nothing_else(gpu):
    table = ei.table_ids(9001, "gaps")
    idx = gpu.VectorIndex(table, _vectors(9001))
    idx.profile_enable(True)
    idx.debug_resolve_ids(ei.id_sets(table)["tenth"])
    prof = idx.profile_read()
    assert set(prof) == RESOLVE_KERNELS and all(v[0] == 1 for v in prof.values()), prof
    idx.debug_resolve_ids(np.zeros(0, np.int32))          # the empty set launches nothing
    assert all(v[0] == 1 for v in idx.profile_read().values())
    idx.profile_enable(False)
    idx.close()


@pytest.mark.parametrize("block", [0, 8])
def test_resolve_after_remove_and_append(gpu, block):
    """remove_rows and append_rows on the handle: the resolve reads the handle's current ids (rows move down, new rows follow)."""
    N = 9001
    table = ei.table_ids(N, "gaps")
    x = _vectors(N + 700)
    idx = gpu.VectorIndex(table, x[:N])
    idx.set_option("resolve_block", block)
    rng = np.random.default_rng(5)
    gone = table[rng.choice(N, 1500, replace=False)]
    assert idx.remove_rows(gone) == 1500
    table = np.setdiff1d(table, gone).astype(np.int32)
    _check_sets(idx, table, 11, "after remove_rows")
    assert idx.debug_resolve_ids(gone).size == 0          # the removed ids are unknown now
    new = (int(table[-1]) + 2 + 5 * np.arange(700)).astype(np.int32)
    idx.append_rows(new, vectors=x[N:N + 700])
    table = np.concatenate([table, new])
    _check_sets(idx, table, 12, "after append_rows")
    assert np.array_equal(idx.debug_resolve_ids(new[::-1]), np.arange(table.size - 700, table.size, dtype=np.int32))
    idx.close()


def test_refusals(gpu):
    import ctypes as C
    lib, P = gpu.load(), gpu._p
    table = ei.table_ids(33, "gaps")
    idx = gpu.VectorIndex(table, _vectors(33))
    out, n = np.full(4, -7, np.int32), C.c_int64(-9)
    ids = table[:4].copy()
    assert lib.freddy_gpu_debug_resolve_ids(None, P(ids), 4, P(out), C.byref(n)) == -1
    assert lib.freddy_gpu_debug_resolve_ids(idx.h, P(ids), -1, P(out), C.byref(n)) == -1
    assert lib.freddy_gpu_debug_resolve_ids(idx.h, None, 4, P(out), C.byref(n)) == -1
    assert lib.freddy_gpu_debug_resolve_ids(idx.h, P(ids), 4, None, C.byref(n)) == -1
    assert lib.freddy_gpu_debug_resolve_ids(idx.h, P(ids), 4, P(out), None) == -1
    assert n.value == -9 and (out == -7).all()
    assert lib.freddy_gpu_debug_resolve_ids(idx.h, P(ids), 4, P(out), C.byref(n)) == 0 and n.value == 4 and out.tolist() == [0, 1, 2, 3]
    idx.close()
