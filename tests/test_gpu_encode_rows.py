"""freddy_gpu_encode_rows (csrc/encode_filter.h): the cells and codes of pinned rows, found as MFMA filter + exact refine, are bit
for bit the oracle's (fo_assign_coarse / fo_encode_pq) and freddy_gpu_encode's -- over the shapes where the tiling can go wrong, at
ties, through the redo, with non-finite values, at small and large magnitudes, with every bracket checked, and after mutations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(300, 12, 1024, 1000),   # the bench shape
          (300, 12, 256, 0),       # flat PQ, one byte per code
          (300, 30, 1000, 0),      # S = 10, K not a multiple of 32
          (24, 6, 31, 1),          # S = 4, K < one MFMA tile, a single cell
          (300, 1, 64, 37),        # S = d, odd C
          (25, 5, 256, 32)]        # the reference's other shipped index shape
CHUNK = 70000                      # rows: more than a chunk of the call (65 536)
CASES = [(s, 70, ((0, 1), (5, 33), (0, 70))) for s in SHAPES] + [((24, 6, 31, 1), 2 * CHUNK + 37, ((0, 2 * CHUNK + 37), (5, 2 * CHUNK)))]


def _tables(d, m, K, C, N, seed=11):
    """seeded Gaussian rows; centroids = distinct seeded Gaussian rows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, d)).astype(np.float32)
    cb = np.ascontiguousarray(rng.standard_normal((K, m, d // m)).astype(np.float32).transpose(1, 0, 2))
    coarse = rng.standard_normal((C, d)).astype(np.float32) if C else None
    return x, cb, coarse


def _window_ok(x, cent):
    """The precondition of redone == 0, from the inputs alone (float64): at every prefix of the centroid order at most 8 centroids
    lie within 8e-4 (|x| + max |c|)^2 -- four times a bracket of 2e-4 -- of the prefix minimum."""
    x, cent = x.astype(np.float64), cent.astype(np.float64)
    D = (x * x).sum(1)[:, None] + (cent * cent).sum(1)[None, :] - 2.0 * x @ cent.T
    w = 8e-4 * (np.sqrt((x * x).sum(1)) + np.sqrt((cent * cent).sum(1)).max()) ** 2
    run = np.minimum.accumulate(D, axis=1)
    return all(((D[:, :k + 1] <= (run[:, k] + w)[:, None]).sum(1) <= 8).all() for k in range(D.shape[1]))


def _expected(oracle, x, cb, coarse):
    cell = None if coarse is None else oracle.assign_coarse(coarse, x)
    res = x if coarse is None else (x - coarse[cell]).astype(np.float32)
    return cell, oracle.encode_pq(cb, res), res


def _same(got, want):
    return (got is None and want is None) or (got.dtype == want.dtype and np.array_equal(got, want))


@pytest.mark.parametrize("shape,N,ranges", CASES, ids=["%dx%d_K%d_C%d_N%d" % (c[0] + (c[1],)) for c in CASES])
def test_shapes_against_the_oracle(oracle, shape, N, ranges):
    from freddy_amd import gpu
    d, m, K, C = shape
    S = d // m
    x, cb, coarse = _tables(d, m, K, C, N)
    cell_o, codes_o, res = _expected(oracle, x, cb, coarse)
    assert C == 0 or _window_ok(x, coarse)
    assert all(_window_ok(res[:, p * S:(p + 1) * S], cb[p]) for p in range(m))
    g_cell, g_codes = gpu.encode(cb, x, coarse=coarse)
    assert _same(g_cell, cell_o) and _same(g_codes, codes_o)
    vi = gpu.VectorIndex(np.arange(1, N + 1, dtype=np.int32), x)
    vi.profile_enable()
    for row0, n in ranges:
        cell, codes = vi.encode_rows(cb, coarse=coarse, row0=row0, n_rows=n)
        assert _same(cell, None if C == 0 else cell_o[row0:row0 + n]) and _same(codes, codes_o[row0:row0 + n]), (row0, n)
        st = vi.last_encode_stats()
        print(shape, row0, n, st)
        assert st["redone"] == 0 and st["violations"] == 0 and st["items"] == n * (m + (C > 0)) and st["candidates"] >= st["items"]
    prof = vi.profile_read()
    assert "encode_filter_kernel" in prof and "assign_coarse_kernel" not in prof and "encode_pq_kernel" not in prof, prof
    vi.close()


@pytest.mark.parametrize("shape", [(24, 6, 31, 1), (25, 1, 40, 0)], ids=["S4", "S25"])
def test_ties_and_near_ties(oracle, shape):
    """duplicated entries (the lowest index wins), entries one ulp apart, rows equal to a centroid, rows midway between two"""
    from freddy_amd import gpu
    d, m, K, C = shape
    x, cb, coarse = _tables(d, m, K, C, 64, seed=5)
    cb[:, 9] = cb[:, 2]; cb[:, 3] = cb[:, 20]                     # duplicates in both index orders
    cb[:, 12] = np.nextafter(cb[:, 11], np.float32(np.inf)); cb[:, 14] = np.nextafter(cb[:, 15], np.float32(-np.inf))
    flat = cb.transpose(1, 0, 2).reshape(K, d)                    # centroid c of every position, side by side
    off = 0 if coarse is None else coarse[0]                      # (C == 1: every residual is x - coarse[0])
    x[0:16] = flat[[2, 9, 3, 20, 11, 12, 14, 15, 0, 1, 30, 5, 6, 7, 8, 10]] + off
    x[16:32] = (flat[np.arange(16)] + flat[np.arange(16) + 1]) * np.float32(0.5) + off
    cell_o, codes_o, _ = _expected(oracle, x, cb, coarse)
    vi = gpu.VectorIndex(np.arange(1, 65, dtype=np.int32), x)
    cell, codes = vi.encode_rows(cb, coarse=coarse)
    assert _same(cell, cell_o) and _same(codes, codes_o)
    assert vi.last_encode_stats()["violations"] == 0
    assert _same(gpu.encode(cb, x, coarse=coarse)[1], codes)
    vi.close()


def test_redo_of_crowded_items(oracle):
    """64 copies of one centroid in one position: the rows near it have more than 16 centroids inside the bracket and are redone
    all-exact; every other item is filtered"""
    from freddy_amd import gpu
    d, m, K = 24, 6, 100
    x, cb, _ = _tables(d, m, K, 0, 96, seed=7)
    cb[2, 10:74] = np.float32(6.0)                    # far from every Gaussian row: only the rows put near it meet the copies
    near = np.arange(0, 96, 3)
    x[near, 8:12] = cb[2, 10] + np.float32(1e-3) * x[near, 8:12]
    _, codes_o, _ = _expected(oracle, x, cb, None)
    assert (np.delete(codes_o[:, 2], near) != 10).all()
    vi = gpu.VectorIndex(np.arange(1, 97, dtype=np.int32), x)
    vi.profile_enable()
    _, codes = vi.encode_rows(cb)
    st, prof = vi.last_encode_stats(), vi.profile_read()
    assert _same(codes, codes_o) and (codes[near, 2] == 10).all()
    assert 0 < st["redone"] <= near.size and st["violations"] == 0, st
    assert prof["encode_pq_kernel"][0] == 1 and prof["encode_filter_kernel"][0] == 1 and st["candidates"] >= 96 * m - near.size, (prof, st)
    vi.close()


@pytest.mark.parametrize("name", ["16_in_tile0", "17_in_tile0", "16_in_last_tile", "17_in_last_tile", "compaction_12_then_10", "33_in_one_tile"])
def test_list_mechanics_over_three_tiles(name):
    """Steps b and c of encode_filter_kernel (the append `a - eps <= U`, the compaction `if (av - eps <= Urow)` of a list above ENC_KEEP,
    `have > ENC_CAP`) at m = 6, S = 4, K = 300: 16 copies of the nearest centroid are filtered and the lowest index wins, 17 are redone,
    in tile 0 and in the last tile; 12 farther copies in tile 0 are compacted away by 10 nearer ones in tile 1; 33 arrivals in one
    tile are redone.  `redone` is the count tests/assign_filter_inputs.py predicts with the header's bracket (proven separated in
    tests/test_assign_filter_inputs_cpu.py)."""
    import assign_filter_inputs as fi
    from freddy_amd import gpu
    x, cb, winner, redone = fi.encode_cases()[name]
    S = fi.ENC_D // fi.ENC_M
    want = gpu.encode(cb, x)
    vi = gpu.VectorIndex(np.arange(1, len(x) + 1, dtype=np.int32), x)
    got = vi.encode_rows(cb)
    st = vi.last_encode_stats()
    assert _same(got[0], want[0]) and _same(got[1], want[1]), (name, st)
    assert (got[1][list(fi.ENC_NEAR), fi.ENC_POS] == winner).all(), name
    predicted = sum(int(fi.enc_predicted_redo(x[:, p * S:(p + 1) * S], cb[p]).sum()) for p in range(fi.ENC_M))
    assert predicted == (len(fi.ENC_NEAR) if redone else 0)
    assert st["redone"] == predicted and st["violations"] == 0 and st["items"] == len(x) * fi.ENC_M, (name, st)
    vi.set_option("encode_refine_all", 1)                    # every bracket of the same input checked
    again = vi.encode_rows(cb)
    st = vi.last_encode_stats()
    assert _same(again[1], want[1]) and st["redone"] == predicted and st["violations"] == 0 and st["checked"] > 0, (name, st)
    vi.close()


@pytest.mark.parametrize("kind", ["bad_rows", "nan_centroid_0", "nan_centroid_5", "nan_coarse", "scale_-40", "scale_20"])
def test_non_finite_values_and_magnitudes(kind):
    from freddy_amd import gpu
    d, m, K, C = 24, 6, 31, 3
    x, cb, coarse = _tables(d, m, K, C, 70, seed=3)
    if kind == "bad_rows":
        x[3, 5] = np.nan; x[9, 0] = np.inf; x[17, 23] = -np.inf; x[40, 7] = 3e38; x[41, 8] = -3e38
    elif kind.startswith("nan_centroid"):
        cb[4, int(kind[-1]), 1] = np.nan
    elif kind == "nan_coarse":
        coarse[1, 2] = np.nan
    else:
        f = np.float32(2.0) ** int(kind.split("_")[1])
        x, cb, coarse = x * f, cb * f, coarse * f
    want = gpu.encode(cb, x, coarse=coarse)
    vi = gpu.VectorIndex(np.arange(1, 71, dtype=np.int32), x)
    got = vi.encode_rows(cb, coarse=coarse)
    st = vi.last_encode_stats()
    assert _same(got[0], want[0]) and _same(got[1], want[1]), (kind, st)
    assert st["violations"] == 0
    if kind.startswith("scale"):
        assert st["redone"] == 0, st
    vi.close()


@pytest.mark.parametrize("shape", [(24, 6, 31, 1), (25, 5, 256, 32)], ids=["S4", "S5"])
def test_refine_all_checks_every_bracket(shape):
    from freddy_amd import gpu
    d, m, K, C = shape
    n = 70
    x, cb, coarse = _tables(d, m, K, C, n)
    vi = gpu.VectorIndex(np.arange(1, n + 1, dtype=np.int32), x)
    off = vi.encode_rows(cb, coarse=coarse)
    vi.set_option("encode_refine_all", 1)
    on = vi.encode_rows(cb, coarse=coarse)
    st = vi.last_encode_stats()
    assert st["checked"] == n * (m * K + C) and st["violations"] == 0 and st["redone"] == 0, st
    assert _same(on[0], off[0]) and _same(on[1], off[1])
    vi.close()


def test_mutations_and_handle_refusals():
    from freddy_amd import gpu
    d, m, K, C = 24, 6, 31, 3
    x, cb, coarse = _tables(d, m, K, C, 150, seed=9)
    vi = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), x[:100])
    vi.append_rows(np.arange(101, 151, dtype=np.int32), vectors=x[100:])
    gone = np.array([2, 64, 65, 120, 150], np.int32)
    assert vi.remove_rows(gone) == gone.size
    rest = np.delete(x, gone - 1, axis=0)
    want = gpu.encode(cb, rest, coarse=coarse)
    got = vi.encode_rows(cb, coarse=coarse)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert vi.encode_rows(cb, coarse=coarse, row0=vi.N, n_rows=0)[1].shape == (0, m)
    for kw, code in ((dict(row0=1, n_rows=vi.N), -1), (dict(row0=-1, n_rows=1), -1)):
        with pytest.raises(gpu.FreddyGpuError) as e:
            vi.encode_rows(cb, coarse=coarse, **kw)
        assert e.value.code == code
    with pytest.raises(gpu.FreddyGpuError) as e:
        vi.encode_rows(cb[:, :, :3])                         # desc->d = 18 on a 24-d handle
    assert e.value.code == -1
    # a handle of another kind: FREDDY_E_KIND, as every call on a vector handle answers it
    pq = gpu.PQIndex(cb, np.arange(1, 101, dtype=np.int32), want[1][:100])
    with pytest.raises(gpu.FreddyGpuError) as e:
        gpu.VectorIndex.encode_rows(pq, cb, n_rows=1)
    assert e.value.code == -4 and "wrong kind" in str(e.value)
    pq.close()
    # a poisoned handle (an allocation of update_rows fails after its first write, tried from the last one down): FREDDY_E_HIP
    c0 = gpu.alloc_stats().calls
    vi.update_rows(np.arange(1, 41, dtype=np.int32), vectors=x[60:100])
    n_alloc = gpu.alloc_stats().calls - c0
    vi.close()
    for nth in range(n_alloc, 0, -1):
        bad = gpu.VectorIndex(np.arange(1, 101, dtype=np.int32), x[:100])
        gpu.alloc_fail_nth(nth)
        try:
            bad.update_rows(np.arange(1, 41, dtype=np.int32), vectors=x[60:100])
        except gpu.FreddyGpuError:
            pass
        finally:
            gpu.alloc_fail_nth(0)
        try:
            bad.encode_rows(cb, coarse=coarse)
        except gpu.FreddyGpuError as err:
            assert err.code == -2 and "unpin it and pin again" in str(err)
            break
        finally:
            bad.close()
    else:
        raise AssertionError("no failed allocation of update_rows poisoned the handle")


def _crowd(x, cb):
    cb[0, 10:30] = np.float32(6.0)
    x[::3] = cb[0, 10] + np.float32(1e-3) * x[::3]


ALL_EXACT = {   # name: (d, m, K, C), what is done to the tables, whether the filter kernel still runs
    "m1_nan_centroid": ((25, 1, 40, 0), lambda x, cb: cb.__setitem__((0, 5, 1), np.nan), True),    # m = 1, K % 64 != 0: the redo's codebook slice
    "m1_crowded": ((25, 1, 40, 0), _crowd, True),
    "wide_S": ((600, 1, 100, 0), None, False),                                                   # S > 512: the whole call all-exact
    "wide_d_coarse": ((600, 6, 40, 5), None, False),                                             # d > 512 with a coarse quantizer
}


@pytest.mark.parametrize("name", list(ALL_EXACT))
def test_all_exact_paths_inside_the_call(name):
    """what the filter does not answer goes through freddy_gpu_encode's kernels in the same call, for every shape that call accepts"""
    from freddy_amd import gpu
    (d, m, K, C), change, filtered = ALL_EXACT[name]
    x, cb, coarse = _tables(d, m, K, C, 70, seed=13)
    if change:
        change(x, cb)
    want = gpu.encode(cb, x, coarse=coarse)
    vi = gpu.VectorIndex(np.arange(1, 71, dtype=np.int32), x)
    vi.profile_enable()
    got = vi.encode_rows(cb, coarse=coarse)
    st, prof = vi.last_encode_stats(), vi.profile_read()
    assert _same(got[0], want[0]) and _same(got[1], want[1]), st
    assert "encode_pq_kernel" in prof and ("encode_filter_kernel" in prof) == filtered, prof
    assert 0 < st["redone"] and (filtered or st["redone"] == st["items"] == 70 * (m + (C > 0))), st
    vi.close()


def test_tables_from_pinned_rows():
    from freddy_amd import gpu, index_build as ib
    d, m, K, C = 24, 6, 31, 3
    x, cb, coarse = _tables(d, m, K, C, 70, seed=2)
    cb2 = _tables(d, m, K, 0, 1, seed=4)[1]
    vi = gpu.VectorIndex(np.arange(1, 71, dtype=np.int32), x)
    t = ib.build_tables_from_pinned(vi, cb2, coarse=coarse, ivf_codebook=cb)
    cell, codes = gpu.encode(cb, x, coarse=coarse)
    order = np.argsort(cell, kind="stable")
    assert _same(t["pq"]["codes"], gpu.encode(cb2, x)[1]) and np.array_equal(t["pq"]["ids"], np.arange(1, 71))
    assert np.array_equal(t["ivf"]["ids"], order + 1) and _same(t["ivf"]["codes"], codes[order]) and _same(t["ivf"]["coarse_id"], cell)
    assert np.array_equal(np.diff(t["ivf"]["list_off"]), np.bincount(cell, minlength=C))
    vi.close()
