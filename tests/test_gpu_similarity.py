"""-m gpu tests of the similarities by row id (csrc/similarity.h): freddy_gpu_similarity_pairs / _matrix / _join against the numpy model
of tests/similarity_model.py, bit for bit (a NaN is any NaN), at the shapes of tests/similarity_inputs.py; against the exact join and
the exact assign on the same handle; in several passes; after remove_rows / update_rows / append_rows; with non-finite rows; and the
kernels' names in the profile."""
import numpy as np
import pytest

import similarity_inputs as si
import similarity_model as sm
import util

pytestmark = pytest.mark.gpu

MATRIX_KERNELS = {"sim_rows_kernel", "sim_matrix_kernel"}
JOIN_KERNELS = MATRIX_KERNELS | {"sim_count_kernel", "sim_scan_kernel"}


@pytest.fixture(scope="module")
def handles():
    """one pinned table per dimension, made on first use"""
    from freddy_amd import gpu
    made = {}

    def get(d):
        if d not in made:
            ids, x = si.table(d)
            made[d] = (gpu.VectorIndex(ids, x), ids, x)
        return made[d]
    yield get
    for vec, _, _ in made.values():
        vec.close()


def _same_matrix(got, exp, what):
    assert sm.same_floats(got[0], exp[0]), f"{what}: values differ at {np.argwhere(got[0].view(np.uint32) != exp[0].view(np.uint32))[:5].tolist()}"
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), f"{what}: known arrays differ"


def _same_join(got, exp, what):
    assert got[3] == exp[3], f"{what}: total {got[3]}, the model has {exp[3]}"
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), f"{what}: positions or their order differ"
    assert sm.same_floats(got[2], exp[2]), f"{what}: values differ"


def _profiled(vec, call):
    vec.profile_enable(True)
    out = call()
    names = vec.profile_read()
    vec.profile_enable(False)
    return out, names


# ---- against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", si.DIMS)
def test_pairs_equal_the_model(handles, d):
    vec, ids, x = handles(d)
    for n in si.PAIR_N:
        a, b = si.pair_case(d, n)
        (sim, known), names = _profiled(vec, lambda: vec.similarity_pairs(a, b))
        esim, eknown = sm.pairs(ids, x, a, b)
        assert np.array_equal(known, eknown), (d, n)
        assert sm.same_floats(sim, esim), (d, n, np.flatnonzero(sim.view(np.uint32) != esim.view(np.uint32))[:8])
        assert (sim[~known] == 0).all() and not np.signbit(sim[~known]).any()
        assert set(names) == ({"sim_pairs_kernel"} if eknown.any() else set()), (d, n, names)
    if d == 300:   # v1 is the row of ids_a: the same bits either way round for finite rows, and a row against itself
        a, b = si.pair_case(d, 130)
        assert np.array_equal(vec.similarity_pairs(b, a)[0].view(np.uint32), vec.similarity_pairs(a, b)[0].view(np.uint32))


@pytest.mark.parametrize("d", si.DIMS)
def test_matrix_and_join_equal_the_model(handles, d):
    vec, ids, x = handles(d)
    for na in si.MATRIX_NA:
        for nb in si.MATRIX_NB:
            a, b = si.matrix_case(d, na, nb)
            what = f"d={d} na={na} nb={nb}"
            got, names = _profiled(vec, lambda: vec.similarity_matrix(a, b))
            exp = sm.matrix(ids, x, a, b)
            _same_matrix(got, exp, what)
            launched = exp[1].any() and exp[2].any()
            assert set(names) == ((MATRIX_KERNELS | {"query_gather"}) if launched else set()), (what, names)
            thr = si.join_threshold(*exp)
            gj, names = _profiled(vec, lambda: vec.similarity_join(a, b, thr, max_pairs=na * nb))
            ej = sm.join_of(*exp, thr)
            _same_join(gj, ej, what + f" thr={thr}")
            if launched:
                assert set(names) == JOIN_KERNELS | {"query_gather"} | ({"sim_fill_kernel"} if ej[3] else set()), (what, names)
                assert names["sim_matrix_kernel"][0] == 1, "the join computes every chain once"


@pytest.mark.parametrize("d", [30, 33])
def test_rows_of_120_bytes_and_a_tail_of_one_dimension(d):
    """The two widths si.DIMS leaves out: d = 30 (rows aligned to 8 bytes, not 16: the scalar loads with every piece but the last
    whole) and d = 33 (one full step of 32 dimensions and a tail of one); 300 rows, 65 pairs, a matrix of 17 x 65."""
    from freddy_amd import gpu
    ids, x = si.table(d, 300)
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(d)
    a, b = si.draw_ids(ids, 65, rng), si.draw_ids(ids, 65, rng)
    sim, known = vec.similarity_pairs(a, b)
    esim, eknown = sm.pairs(ids, x, a, b)
    assert np.array_equal(known, eknown) and eknown.any() and not eknown.all()
    assert sm.same_floats(sim, esim), (d, np.flatnonzero(sim.view(np.uint32) != esim.view(np.uint32))[:8])
    _same_matrix(vec.similarity_matrix(a[:17], b), sm.matrix(ids, x, a[:17], b), f"d={d} na=17 nb=65")
    vec.close()


@pytest.mark.parametrize("d", [12, 7])
def test_the_constructed_join(d):
    """similarities equal to the threshold and one ulp above, NaNs, +0.0 against -0.0, blocks of 0 / 1 / 64 matches, the last lane of a
    block followed by lane 0 of the next (tests/test_similarity_inputs_cpu.py proves that the case holds all of them)"""
    from freddy_amd import gpu
    ids, x, a_ids, b_ids, thresholds = si.constructed(d)
    vec = gpu.VectorIndex(ids, x)
    exp = sm.matrix(ids, x, a_ids, b_ids)
    _same_matrix(vec.similarity_matrix(a_ids, b_ids), exp, f"constructed d={d}")
    for thr in thresholds:
        for a in (a_ids, exp_vectors(ids, x, a_ids)):
            em = exp if a is a_ids else sm.matrix(ids, x, a, b_ids)
            _same_join(vec.similarity_join(a, b_ids, thr), sm.join_of(*em, thr), f"constructed d={d} thr={thr!r}")
    vec.set_option("similarity_pass_bytes", 1)          # 16 rows per pass at least: one pass here; then five rows repeated over three passes
    a3 = np.tile(a_ids, 8)[:37]
    _same_join(vec.similarity_join(a3, b_ids, si.THR), sm.join(ids, x, a3, b_ids, si.THR), f"constructed d={d}, three passes")
    vec.close()


def exp_vectors(ids, x, a_ids):
    """the rows of the known a_ids as vectors (an unknown id becomes a zero vector: a known row of its own)"""
    r = sm.rows_of(ids, a_ids)
    v = np.zeros((r.size, x.shape[1]), np.float32)
    v[r >= 0] = x[r[r >= 0]]
    return v


# ---- ids ---------------------------------------------------------------------------------------------------------------------------
def test_calls_in_which_no_id_has_a_row_launch_nothing(handles):
    vec, ids, x = handles(25)
    bad = si.unknown_ids(ids)
    good = ids[:70]
    (sim, known), names = _profiled(vec, lambda: vec.similarity_pairs(np.resize(bad, 70), good))
    assert not names and not known.any() and not sim.any()
    for a, b in ((bad, good), (good, bad), (bad, bad)):
        (out, ka, kb), names = _profiled(vec, lambda: vec.similarity_matrix(a, b))
        assert not names and not out.any() and out.shape == (a.size, b.size)
        assert np.array_equal(ka, sm.rows_of(ids, a) >= 0) and np.array_equal(kb, sm.rows_of(ids, b) >= 0)
        (ia, ib, s, total), names = _profiled(vec, lambda: vec.similarity_join(a, b, -np.inf))
        assert not names and total == 0 and ia.size == 0
    (out, ka, kb), names = _profiled(vec, lambda: vec.similarity_matrix(x[:3], bad))       # vectors against unknown ids
    assert not names and not out.any() and ka.all() and not kb.any()
    # empty sides
    assert vec.similarity_pairs([], [])[0].size == 0
    assert vec.similarity_matrix(np.zeros(0, np.int32), good)[0].shape == (0, 70) and vec.similarity_matrix(good, [])[0].shape == (70, 0)
    assert vec.similarity_join(np.zeros((0, 25), np.float32), good, 0.0)[3] == 0


@pytest.mark.parametrize("d", [300, 25])
def test_a_by_vectors_equals_a_by_ids(handles, d):
    vec, ids, x = handles(d)
    rng = np.random.default_rng(d)
    a = ids[rng.integers(0, ids.size, size=33)]
    b = si.draw_ids(ids, 200, rng)
    by_ids = vec.similarity_matrix(a, b)
    by_vec = vec.similarity_matrix(x[sm.rows_of(ids, a)], b)
    _same_matrix(by_vec, by_ids, f"d={d} vectors against ids")
    thr = si.join_threshold(*by_ids)
    _same_join(vec.similarity_join(x[sm.rows_of(ids, a)], b, thr), vec.similarity_join(a, b, thr), f"d={d} join, vectors against ids")
    # vectors that are no rows
    v = (x[rng.integers(0, ids.size, size=17)] * np.float32(0.5) + x[rng.integers(0, ids.size, size=17)] * np.float32(0.25)).astype(np.float32)
    got, names = _profiled(vec, lambda: vec.similarity_matrix(v, b))
    _same_matrix(got, sm.matrix(ids, x, v, b), f"d={d} free vectors")
    assert set(names) == MATRIX_KERNELS, names                                           # staged, not gathered
    _same_join(vec.similarity_join(v, b, 0.1), sm.join(ids, x, v, b, 0.1), f"d={d} free vectors, join")


# ---- passes and max_pairs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [300, 7])
def test_three_passes_equal_one(handles, d):
    vec, ids, x = handles(d)
    a, b = si.matrix_case(d, 33, 200)
    a[[15, 16, 32]] = ids[[100, 200, 300]]                                             # known rows at both sides of the pass boundaries
    one = vec.similarity_matrix(a, b)
    thr = si.join_threshold(*one, frac=0.3)
    one_join = vec.similarity_join(a, b, thr)
    vec.set_option("similarity_pass_bytes", 16 * 200 * 4)
    try:
        got, names = _profiled(vec, lambda: vec.similarity_matrix(a, b))
        assert names["sim_matrix_kernel"][0] == 3 and names["sim_rows_kernel"][0] == 1, names
        _same_matrix(got, one, f"d={d} three passes")
        gj, names = _profiled(vec, lambda: vec.similarity_join(a, b, thr))            # (a count call, then the pairs: two calls of three passes)
        assert names["sim_matrix_kernel"][0] == 6 and names["sim_scan_kernel"][0] == 6, names
        _same_join(gj, one_join, f"d={d} join in three passes")
        exp = sm.join(ids, x, a, b, thr)
        _same_join(gj, exp, f"d={d} join in three passes against the model")
        assert (exp[0] < 16).any() and (exp[0] >= 16).any() and (exp[0] >= 32).any(), "matches on both sides of every pass boundary"
        cut = int((exp[0] < 16).sum()) + 1                                             # one match into the second pass
        _same_join(vec.similarity_join(a, b, thr, max_pairs=cut), sm.join(ids, x, a, b, thr, cut), f"d={d} max_pairs ends inside pass two")
    finally:
        vec.set_option("similarity_pass_bytes", 0)


def test_max_pairs(handles):
    vec, ids, x = handles(32)
    a, b = si.matrix_case(32, 17, 65)
    exp = sm.matrix(ids, x, a, b)
    thr = si.join_threshold(*exp, frac=0.2)
    total = sm.join_of(*exp, thr)[3]
    assert total > 5
    full = vec.similarity_join(a, b, thr)
    for cap in (0, 1, total - 1, total, total + 5):
        got = vec.similarity_join(a, b, thr, max_pairs=cap)
        _same_join(got, sm.join_of(*exp, thr, cap), f"max_pairs={cap}")
        n = min(cap, total)
        assert got[3] == total and got[0].size == n
        assert np.array_equal(got[0], full[0][:n]) and np.array_equal(got[1], full[1][:n]) and sm.same_floats(got[2], full[2][:n])   # the prefix
    (_, names) = _profiled(vec, lambda: vec.similarity_join(a, b, thr, max_pairs=0))
    assert "sim_fill_kernel" not in names and "sim_count_kernel" in names, names       # a count call writes no pairs


# ---- against the entry points that rank ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [300, 25])
def test_matrix_rows_begin_with_the_exact_joins_lists(handles, d):
    vec, ids, x = handles(d)
    rng = np.random.default_rng(3 + d)
    qs = x[rng.choice(ids.size, 5, replace=False)]
    b = rng.choice(ids, 300, replace=False).astype(np.int32)
    out, ka, kb = vec.similarity_matrix(qs, b)
    ji, js = vec.join(qs, 20, b)
    for i in range(5):
        order = np.lexsort((b, -out[i].astype(np.float64)))                             # similarity DESC, id ASC (finite rows)
        assert np.array_equal(b[order][:20], ji[i]), (d, i)
        assert np.array_equal(out[i][order][:20].view(np.uint32), js[i].view(np.uint32)), (d, i)


@pytest.mark.parametrize("d", [300, 25])
def test_the_column_argmax_is_the_exact_assign(handles, d):
    vec, ids, x = handles(d)
    rng = np.random.default_rng(5 + d)
    qs = np.stack([x[rng.choice(ids.size, 10)].mean(axis=0) for _ in range(17)]).astype(np.float32)
    qs[9] = qs[2]                                                                       # identical queries: the lower index wins
    b = si.draw_ids(ids, 130, rng)
    out, ka, kb = vec.similarity_matrix(qs, b)
    eq, es = sm.assign_of(out, kb)
    gq, gs = vec.assign(qs, b)
    assert np.array_equal(gq, eq) and np.array_equal(gs.view(np.uint32), es.view(np.uint32))


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [300, 7])
def test_after_mutations_every_call_equals_the_model_and_a_fresh_pin(d):
    from freddy_amd import gpu
    ids0, x0 = si.table(d)
    n0 = 2600
    ids, x = ids0[:n0].copy(), x0[:n0].copy()
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(d)

    def check(what):
        a, b = si.draw_ids(ids0, 33, rng), si.draw_ids(ids0, 200, rng)                   # (ids of the whole source: removed and not yet appended ones are unknown)
        pa, pb = si.draw_ids(ids0, 130, rng), si.draw_ids(ids0, 130, rng)
        fresh = gpu.VectorIndex(ids, x)
        thr = None
        for ix, name in ((vec, "the mutated handle"), (fresh, "a fresh pin")):
            sim, known = ix.similarity_pairs(pa, pb)
            es, ek = sm.pairs(ids, x, pa, pb)
            assert np.array_equal(known, ek) and sm.same_floats(sim, es), (what, name)
            exp = sm.matrix(ids, x, a, b)
            _same_matrix(ix.similarity_matrix(a, b), exp, f"{what}, {name}")
            thr = si.join_threshold(*exp)
            _same_join(ix.similarity_join(a, b, thr), sm.join_of(*exp, thr), f"{what}, {name}")
        fresh.close()

    gone = np.concatenate([ids[rng.choice(n0, 300, replace=False)], ids[:3], ids[-2:]]).astype(np.int32)
    vec.remove_rows(gone)
    keep = ~np.isin(ids, gone)
    ids, x = ids[keep], x[keep]
    check("after remove_rows")
    rows = rng.choice(ids.size, 200, replace=False)
    newv = x0[rng.choice(len(x0), 200, replace=False)] * np.float32(0.5)
    vec.update_rows(ids[rows], vectors=newv)
    x[rows] = newv
    check("after update_rows")
    vec.append_rows(ids0[n0:], vectors=x0[n0:])
    ids, x = np.concatenate([ids, ids0[n0:]]), np.concatenate([x, x0[n0:]])
    check("after append_rows")
    vec.close()


# ---- non-finite rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [300, 25])
def test_non_finite_rows_leave_the_healthy_entries_alone(handles, d):
    from freddy_amd import gpu
    clean, ids, x = handles(d)
    _, px, rows = si.poisoned_table(d)
    vec = gpu.VectorIndex(ids, px)
    rng = np.random.default_rng(9 + d)
    a = np.concatenate([ids[rows], ids[rng.integers(0, ids.size, size=25)]]).astype(np.int32)      # 33 A rows, eight of them poisoned
    b = np.concatenate([ids[rows], si.draw_ids(ids, 192, rng)]).astype(np.int32)
    exp = sm.matrix(ids, px, a, b)
    got = vec.similarity_matrix(a, b)
    _same_matrix(got, exp, f"d={d} poisoned table")
    assert np.isnan(exp[0]).any() and np.isinf(exp[0]).any()
    ha, hb = ~np.isin(a, ids[rows]), ~np.isin(b, ids[rows])
    ref = clean.similarity_matrix(a, b)
    assert np.array_equal(got[0][np.ix_(ha, hb)].view(np.uint32), ref[0][np.ix_(ha, hb)].view(np.uint32)), "a healthy entry changed with its neighbours' poison"
    for thr in (si.join_threshold(*exp), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)):
        ej = sm.join_of(*exp, thr)
        _same_join(vec.similarity_join(a, b, thr), ej, f"d={d} poisoned table thr={thr!r}")
    assert np.isnan(sm.join_of(*exp, np.float32(np.inf))[2]).all() and sm.join_of(*exp, np.float32(np.inf))[3] > 0   # only NaNs pass +inf
    pa, pb = np.resize(a, 130), np.resize(b[::-1], 130)
    sim, known = vec.similarity_pairs(pa, pb)
    es, ek = sm.pairs(ids, px, pa, pb)
    assert np.array_equal(known, ek) and sm.same_floats(sim, es)
    vec.close()


# ---- soak ----------------------------------------------------------------------------------------------------------------------------------
def test_soak_of_drawn_shapes():
    from freddy_amd import gpu
    for k, (d, na, nb, npairs, by_vectors, frac) in enumerate(si.soak_cases()):
        rng = np.random.default_rng(100 + k)
        n = int(rng.integers(200, 900))
        x = util.shape_corpus(n, d, seed=k).numpy().astype(np.float32)
        ids = (np.cumsum(rng.integers(1, 5, size=n)) + 5).astype(np.int32)
        vec = gpu.VectorIndex(ids, x)
        what = f"soak {k}: d={d} n={n} na={na} nb={nb}"
        pa, pb = si.draw_ids(ids, npairs, rng), si.draw_ids(ids, npairs, rng)
        sim, known = vec.similarity_pairs(pa, pb)
        es, ek = sm.pairs(ids, x, pa, pb)
        assert np.array_equal(known, ek) and sm.same_floats(sim, es), what
        b = si.draw_ids(ids, nb, rng)
        a = (x[rng.integers(0, n, size=na)] * np.float32(0.75)).astype(np.float32) if by_vectors else si.draw_ids(ids, na, rng)
        if k % 4 == 1:
            vec.set_option("similarity_pass_bytes", 4 * nb * 16 * int(rng.integers(1, 4)))
        exp = sm.matrix(ids, x, a, b)
        _same_matrix(vec.similarity_matrix(a, b), exp, what)
        thr = si.join_threshold(*exp, frac=frac) if frac else np.float32(2.0)
        ej = sm.join_of(*exp, thr)
        _same_join(vec.similarity_join(a, b, thr), ej, what + f" thr={thr}")
        cap = int(rng.integers(0, ej[3] + 2))
        _same_join(vec.similarity_join(a, b, thr, max_pairs=cap), sm.join_of(*exp, thr, cap), what + f" max_pairs={cap}")
        vec.close()
