"""-m gpu: the statistics row of a pinned ivpq handle -- freddy_gpu_set_statistics / freddy_gpu_get_statistics /
freddy_gpu_create_statistics (include/freddy_gpu.h; kernels in postgres-word2vec_amd/csrc/stat_kernels.h).

create_statistics is compared bit for bit (view(uint32)) with the numpy model tests/statistics_model.py on every path of the
count kernel: affine ids and ids with gaps (the binary search), 4 cells (every atomic collides), 16 cells, and the smallest
multi-index above the LDS threshold (k_coarse = 65: 4225 cells, counted with global atomics).  set_statistics is checked where
it matters: the kNN-join afterwards must answer as the CPU oracle over a table with that row and as a fresh pin with it --
lists, distance bits, iterations and the rows of the cells taken -- on inputs tests/test_statistics_inputs_cpu.py proves to
answer differently under the two rows.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import statistics_inputs as si
import statistics_model as sm
import test_gpu_mutation as tm
import update_model as um
import util

pytestmark = pytest.mark.gpu

E_ARG = tm.E_ARG
N = 20000
# (k_coarse, ids with gaps): 16 cells affine / binary search, 4 cells, 4225 cells (> STAT_LDS_CELLS = 4096)
PATHS = {"kc4-affine": (4, False), "kc4-gaps": (4, True), "kc2-collide": (2, False), "kc65-global": (65, False), "kc65-global-gaps": (65, True)}


@pytest.fixture(scope="module")
def gpu():
    from freddy_amd import gpu as g
    g.load()
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_row(got, exp, what):
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    bad = np.nonzero(_bits(got) != _bits(exp))[0]
    assert bad.size == 0, (what, "entries", bad[:5].tolist(), got[bad[:5]].tolist(), exp[bad[:5]].tolist())


@pytest.fixture(scope="module")
def pinned(gpu):
    """path -> (pinned handle, ids, cell, cells, the row it was pinned with); each path is pinned once for the module"""
    have = {}

    def get(path):
        if path not in have:
            kc, gaps = PATHS[path]
            t = util.shape_ivpq_tables(64, 8, 16, kc, N)
            ids = t["ids"]
            if gaps:   # strictly ascending with steps of 1 .. 3, starting above 5: unknown ids below, between and above
                ids = (5 + np.cumsum(np.random.default_rng(kc).integers(1, 4, N))).astype(np.int32)
            idx = gpu.IVPQIndex(t["codebook"], t["coarse"], ids, t["coarse_id"], t["codes"], None, t["stats"])
            have[path] = (idx, ids, t["coarse_id"], kc * kc, t["stats"])
        return have[path]

    yield get
    for idx, *_ in have.values():
        idx.close()


def _check(idx, ids, cell, cells, column, what):
    got, matched = idx.create_statistics(column)
    exp, total = sm.create_statistics(ids, cell, cells, column)
    assert matched == total, (what, matched, total)
    _same_row(got, exp, what)


@pytest.mark.parametrize("path", list(PATHS))
def test_create_statistics_equals_the_model(pinned, path):
    idx, ids, cell, cells, pinned_row = pinned(path)
    rng = np.random.default_rng(3)
    gaps = PATHS[path][1]
    assert (int(ids[-1]) - int(ids[0]) != N - 1) == gaps
    got, matched = idx.create_statistics()
    assert matched == N
    _same_row(got, sm.create_statistics(ids, cell, cells)[0], "every pinned row once")
    absent = np.setdiff1d(np.arange(int(ids[0]), int(ids[-1])), ids)[:50]
    assert (absent.size > 0) == gaps
    column = np.concatenate([ids[rng.integers(0, N, 3000)], np.repeat(ids[[0, N - 1, 777]], [5, 9, 300]), ids[:64],
                             [int(ids[0]) - 1, 0, -7, -2 ** 31, int(ids[-1]) + 1, 2 ** 31 - 1], absent])
    column = column[rng.permutation(column.size)]
    _check(idx, ids, cell, cells, column, "duplicates and unknown ids below, between and above the pinned ids")
    c0 = int(cell[123])
    _check(idx, ids, cell, cells, np.repeat(ids[cell == c0], 2), "every entry in one cell")
    _same_row(idx.statistics(), pinned_row, "nothing was installed")


@pytest.mark.parametrize("path", ["kc4-affine", "kc4-gaps"])
def test_list_lengths_around_a_workgroup_and_a_pass(gpu, pinned, path):
    idx, ids, cell, cells, _ = pinned(path)
    rng = np.random.default_rng(4)
    pool = np.concatenate([ids, [int(ids[-1]) + 5, int(ids[0]) - 2]])
    first = ids[0:1] if path == "kc4-affine" else ids[-1:]
    for n in (1, 255, 256, 257, gpu.STAT_PASS + 1):
        column = first if n == 1 else pool[rng.integers(0, pool.size, n)]
        if n > 1:
            column[-1] = ids[4321]      # (the entry beyond the pass boundary has a row)
        _check(idx, ids, cell, cells, column, f"{n} ids")


def test_a_count_above_2_pow_24_in_one_call(pinned):
    """One id 2^24 + 3 times and a few others, 68 MB of ids in five passes: the smallest input at which 32-bit float counters, a
    float division or a pass boundary can go wrong."""
    idx, ids, cell, cells, _ = pinned("kc4-affine")
    rep = 2 ** 24 + 3
    column = np.full(rep + 40, ids[1000], np.int32)
    others = np.arange(0, 40) * 37
    column[rep:] = ids[others]
    count = np.bincount(cell[others], minlength=cells).astype(np.int64)
    count[cell[1000]] += rep
    exp = sm.row_from_counts(count, rep + 40)
    assert _bits(exp)[cell[1000]] != _bits(np.float32(count[cell[1000]]) / np.float32(rep + 40)), "the case does not bite"
    got, matched = idx.create_statistics(column)
    assert matched == rep + 40
    _same_row(got, exp, "2^24 + 3 entries of one row")


def test_errors_leave_the_row_as_it_was(gpu, pinned):
    idx, ids, cell, cells, pinned_row = pinned("kc4-gaps")
    lib = idx.lib
    some = np.ascontiguousarray(ids[:5])
    buf, row = np.full(cells + 1, -5.0, np.float32), np.zeros(cells + 3, np.float32)
    matched = C.c_int64(-9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def unchanged(what):
        _same_row(idx.statistics(), pinned_row, what)
        assert (buf == -5.0).all() and matched.value == -9, (what, "an output was written")

    for n in (cells, cells + 2, 0, -1):
        assert lib.freddy_gpu_set_statistics(idx.h, p(row), n) == -1, n
        msg = lib.freddy_gpu_last_error().decode()
        assert str(n) in msg and str(cells + 1) in msg, msg
        assert lib.freddy_gpu_get_statistics(idx.h, p(row), n) == -1, n
        unchanged(f"n_stats = {n}")
    assert lib.freddy_gpu_set_statistics(idx.h, None, cells + 1) == -1
    assert lib.freddy_gpu_get_statistics(idx.h, None, cells + 1) == -1
    assert lib.freddy_gpu_create_statistics(idx.h, None, C.c_int64(5), 1, p(buf), C.byref(matched)) == -1
    unchanged("ids == NULL with n > 0")
    assert lib.freddy_gpu_create_statistics(idx.h, p(some), C.c_int64(-1), 1, p(buf), C.byref(matched)) == -1
    unchanged("n < 0")
    nobody = np.array([int(ids[0]) - 1, -3, int(ids[-1]) + 1, int(np.setdiff1d(np.arange(int(ids[0]), int(ids[-1])), ids)[0])], np.int32)
    assert lib.freddy_gpu_create_statistics(idx.h, p(nobody), C.c_int64(nobody.size), 1, p(buf), C.byref(matched)) == -1
    assert "total is 0" in lib.freddy_gpu_last_error().decode()
    unchanged("a list with no known id")
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG):
        idx.create_statistics(nobody, install=True)
    with pytest.raises(gpu.FreddyGpuError, match=E_ARG):
        idx.create_statistics(np.zeros(0, np.int32), install=True)
    unchanged("an empty list")
    assert lib.freddy_gpu_set_statistics(None, p(row), cells + 1) == -1
    assert lib.freddy_gpu_get_statistics(None, p(row), cells + 1) == -1
    assert lib.freddy_gpu_create_statistics(None, p(some), C.c_int64(5), 1, p(buf), C.byref(matched)) == -1
    t = util.shape_pq_tables(64, 8, 16, 2000)
    pq = gpu.PQIndex(t["codebook"], t["ids"], t["codes"])
    assert lib.freddy_gpu_set_statistics(pq.h, p(row), cells + 1) == -4
    assert lib.freddy_gpu_get_statistics(pq.h, p(row), cells + 1) == -4
    assert lib.freddy_gpu_create_statistics(pq.h, p(some), C.c_int64(5), 1, p(buf), C.byref(matched)) == -4
    pq.close()
    unchanged("a handle of another kind")


# =======================================================================================
# the row decides what the join answers
# =======================================================================================
def _join(idx, method, k, alpha, use_tl=True):
    gi, gd, it = idx.knn_join(si.queries(), k, si.targets(), alpha, si.PVF, method, use_target_lists=use_tl, confidence=si.CONFIDENCE)
    return gi, gd, it, idx.last_track()["candidate_rows"]


def _equals_oracle(got, oracle, which, method, k, alpha, what):
    exp, eit = si.expected(oracle, which, method, k, alpha)
    assert got[2] == eit, (what, "iterations", got[2], eit)
    util.assert_same_lists(got[0], got[1], exp, what)


@pytest.mark.parametrize("host_traversal", [0, 1])
def test_set_statistics_then_the_join_answers_as_a_fresh_pin_and_the_oracle(gpu, oracle, host_traversal):
    a, b = si.row_a(), si.row_b()
    idx, fresh = gpu.IVPQIndex(*si.pin_args(a)), gpu.IVPQIndex(*si.pin_args(b))
    idx.set_option("join_host_traversal", host_traversal); fresh.set_option("join_host_traversal", host_traversal)
    nbytes = idx.nbytes
    for method in si.METHODS:
        for k, alpha in si.CALLS:
            _equals_oracle(_join(idx, method, k, alpha), oracle, "A", method, k, alpha, f"before the swap: method={method} k={k} alpha={alpha}")
    idx.set_statistics(b)
    assert idx.nbytes == nbytes == fresh.nbytes, "freddy_gpu_index_bytes moved"
    _same_row(idx.statistics(), b, "the device's row after set_statistics")
    for method in si.METHODS:
        for k, alpha in si.CALLS:
            w = f"after the swap: method={method} k={k} alpha={alpha} host_traversal={host_traversal}"
            got, exp = _join(idx, method, k, alpha), _join(fresh, method, k, alpha)
            _equals_oracle(got, oracle, "B", method, k, alpha, w)
            tm._bits_equal(got[:2], exp[:2], w)
            assert got[2:] == exp[2:], (w, "iterations and candidate rows", got[2:], exp[2:])
    # the cells each query took: the handle keeps no per-query record, so every query is asked on its own and the rows of the
    # cells it took (last_track: candidate_rows, summed over its rounds) and its rounds are compared with the fresh pin's
    k, alpha = si.CALLS[0]
    qs, per_query = si.queries(), []
    for q in range(si.Q):
        one = []
        for h in (idx, fresh):
            gi, gd, it = h.knn_join(qs[q:q + 1], k, si.targets(), alpha, si.PVF, 0, confidence=si.CONFIDENCE)
            one.append((gi.tobytes(), gd.tobytes(), it, h.last_track()["candidate_rows"]))
        assert one[0] == one[1], ("query", q, one[0][2:], one[1][2:])
        per_query.append(one[0][3])
    assert len(set(per_query)) > 1, "every query took the same rows: the per-query comparison shows nothing"
    idx.set_statistics(a)       # and back: the row is a setting
    _equals_oracle(_join(idx, 0, *si.CALLS[0]), oracle, "A", 0, *si.CALLS[0], "swapped back to A")
    idx.close(); fresh.close()


def test_the_cached_target_list_survives_the_swap(gpu, oracle):
    """join(T) -> set_statistics -> join(T) with the identical target array: the second call finds its targets resolved and
    bucketed (tl_valid) and must still take the cells row B gives."""
    idx, fresh = gpu.IVPQIndex(*si.pin_args(si.row_a())), gpu.IVPQIndex(*si.pin_args(si.row_b()))
    k, alpha = si.CALLS[0]
    first = _join(idx, 0, k, alpha)
    _equals_oracle(first, oracle, "A", 0, k, alpha, "join(T) with A")
    idx.set_statistics(si.row_b())
    got, exp = _join(idx, 0, k, alpha), _join(fresh, 0, k, alpha)
    _equals_oracle(got, oracle, "B", 0, k, alpha, "join(T) after the swap")
    tm._bits_equal(got[:2], exp[:2], "join(T) after the swap")
    assert got[2:] == exp[2:] and got[2] != first[2], (got[2:], exp[2:], first[2:])
    idx.close(); fresh.close()


def test_the_row_follows_its_table_after_mutations(gpu, oracle):
    """append_rows + remove_rows + update_rows leave the row alone; create_statistics(install=True) brings it back in line, and
    the join then answers as a fresh pin of the mutated tables with the model's row."""
    t = si.tables()
    n0 = 15000
    cells = si.cells()
    old = si.row_a()
    model = um.IVPQModel(t["codebook"], t["coarse"], t["ids"][:n0], t["coarse_id"][:n0], t["codes"][:n0], t["vectors"][:n0], old)
    idx = gpu.IVPQIndex(*model.pin_args())
    rng = np.random.default_rng(8)
    sl = np.arange(n0 + 100, N)      # (a gap: the ids stop being consecutive)
    idx.append_rows(t["ids"][sl], t["coarse_id"][sl], t["codes"][sl], t["vectors"][sl])
    model.append(t["ids"][sl], t["coarse_id"][sl], t["codes"][sl], t["vectors"][sl])
    big = int(np.argmax(np.bincount(model.cell, minlength=cells)))
    gone = model.ids[model.cell == big][::2]
    assert idx.remove_rows(gone) == model.remove(gone) == gone.size
    upd = model.ids[rng.choice(model.N, 2000, replace=False)]
    src = rng.choice(n0, upd.size, replace=False)
    new_cell = np.full(upd.size, (big + 1) % cells, np.int32)
    assert idx.update_rows(upd, coarse_id=new_cell, codes=t["codes"][src], vectors=t["vectors"][src]) == \
        model.update(upd, new_cell, t["codes"][src], t["vectors"][src]) == upd.size
    _same_row(idx.statistics(), old, "the mutation calls leave the row alone")
    exp_row, total = sm.create_statistics(model.ids, model.cell, cells)
    assert total == model.N and not np.array_equal(_bits(exp_row), _bits(old))
    got_row, matched = idx.create_statistics(install=True)
    assert matched == model.N
    _same_row(got_row, exp_row, "the row over the mutated table")
    _same_row(idx.statistics(), exp_row, "the installed row")
    model.stats = exp_row.copy()
    fresh = gpu.IVPQIndex(*model.pin_args())
    assert idx.nbytes == fresh.nbytes
    ot = model.oracle_table(oracle)
    qs = si.queries()
    targets = np.concatenate([model.ids[rng.choice(model.N, 3000, replace=False)], upd[:200], gone[:20]]).astype(np.int32)
    for method in si.METHODS:
        for k, alpha in si.CALLS:
            for hv in (0, 1):
                w = f"after the mutations: method={method} k={k} alpha={alpha} host_traversal={hv}"
                idx.set_option("join_host_traversal", hv); fresh.set_option("join_host_traversal", hv)
                gi, gd, git = idx.knn_join(qs, k, targets, alpha, si.PVF, method, confidence=si.CONFIDENCE)
                fi, fd, fit = fresh.knn_join(qs, k, targets, alpha, si.PVF, method, confidence=si.CONFIDENCE)
                tm._bits_equal((gi, gd), (fi, fd), w)
                assert git == fit, w
                if hv == 0:
                    exp, eit = oracle.ivpq_search_in(ot, qs, k, targets, alpha, si.PVF, method, confidence=si.CONFIDENCE)
                    assert git == eit, (w, git, eit)
                    util.assert_same_lists(gi, gd, exp, w)
    idx.close(); fresh.close()
