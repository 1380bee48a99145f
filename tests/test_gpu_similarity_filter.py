"""-m gpu tests of option similarity_filter (csrc/similarity_filter.h): freddy_gpu_similarity_join as matrix-core filter + exact refine.
Every case holds the triples and the total bit for bit to the numpy model (tests/similarity_model.py: the reference's binary32 chain
and PostgreSQL's float4gt) and to the same call with the option at 0, and reads from the profile which kernel ran."""
import numpy as np
import pytest

import similarity_inputs as si
import similarity_model as sm
import util

pytestmark = pytest.mark.gpu

FILTER, TODAY = "simf_filter_kernel", "sim_matrix_kernel"
DIMS = (16, 20, 300, 512)          # one k-step, a k-step tail, the bench shape, the LDS limit


@pytest.fixture(scope="module")
def handles():
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


def join(vec, a, b, thr, mode, max_pairs=None):
    """the call under option value `mode` -> ((ia, ib, sim, total), profile)"""
    vec.set_option("similarity_filter", mode)
    vec.profile_enable(True)
    out = vec.similarity_join(a, b, thr, max_pairs)
    names = vec.profile_read()
    vec.profile_enable(False)
    vec.set_option("similarity_filter", 0)
    return out, names


def same(got, exp, what):
    assert got[3] == exp[3], f"{what}: total {got[3]}, expected {exp[3]}"
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), f"{what}: positions or their order differ"
    assert sm.same_floats(got[2], exp[2]), f"{what}: values differ"


def check(vec, ids, x, a, b, thr, what, mode=2, max_pairs=None, kernels=(FILTER,), absent=(TODAY,)):
    exp = sm.join(ids, x, a, b, thr, max_pairs)
    got, names = join(vec, a, b, thr, mode, max_pairs)
    same(got, exp, what + " against the model")
    same(got, join(vec, a, b, thr, 0, max_pairs)[0], what + " against option 0")
    a = np.asarray(a)
    ka = sm.rows_of(ids, a) >= 0 if np.issubdtype(a.dtype, np.integer) else np.ones(len(a), bool)
    kb = sm.rows_of(ids, b) >= 0
    if ka.any() and kb.any():
        assert all(k in names for k in kernels) and not any(k in names for k in absent), (what, sorted(names))
    else:
        assert not names, (what, sorted(names))
    return got, names


def threshold(ids, x, a, b, frac=0.02):
    return si.join_threshold(*sm.matrix(ids, x, a, b), frac=frac)


def test_option_belongs_to_a_vector_handle(handles):
    from freddy_amd import gpu
    handles(16)[0].set_option("similarity_filter", 1)          # ("unknown option" without the feature)
    handles(16)[0].set_option("similarity_filter", 0)
    pqt = util.shape_pq_tables(25, 5, 256, 2000)
    pq = gpu.PQIndex(pqt["codebook"], pqt["ids"], pqt["codes"])
    with pytest.raises(gpu.FreddyGpuError, match="error -4"):
        pq.set_option("similarity_filter", 1)
    pq.close()


def test_tile_word_wave_and_chunk_boundaries_with_one_cu(handles):
    """both sides of the 32-row tile, the bitmap word, a wave's 32 columns, one scan chunk; unknown and repeated ids (si.matrix_case)"""
    vec, ids, x = handles(20)
    vec.set_option("grid_cus", 1)
    for na in (1, 31, 33, 129):
        for nb in (1, 31, 65, 8197):
            a, b = si.matrix_case(20, na, nb)
            check(vec, ids, x, a, b, threshold(ids, x, a, b), f"na={na} nb={nb}")
    vec.set_option("grid_cus", 0)


@pytest.mark.parametrize("d", DIMS)
def test_thresholds_at_a_value_of_the_matrix_and_the_self_check(handles, d):
    """t = a value v of the model's own matrix (the pair at t is no match), one ulp below (it is) and above; then check_brackets = 32:
    every known fit pair's bracket holds and the counter equals their number (the table is finite and normalised: every row is fit)"""
    vec, ids, x = handles(d)
    a, b = si.matrix_case(d, 33, 200)
    v = threshold(ids, x, a, b)
    totals = [check(vec, ids, x, a, b, t, f"d={d} t={t!r}")[0][3] for t in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf)))]
    assert totals[0] > totals[1] >= totals[2]
    by_vec = x[sm.rows_of(ids, a[sm.rows_of(ids, a) >= 0])]
    same(join(vec, by_vec, b, v, 2)[0], sm.join(ids, x, by_vec, b, v), f"d={d} A by vectors")
    if d != 20:
        known = int((sm.rows_of(ids, a) >= 0).sum()) * int((sm.rows_of(ids, b) >= 0).sum())
        v0, c0 = vec.bound_violations(), vec.bound_checked()
        vec.set_option("check_brackets", 32)
        check(vec, ids, x, a, b, v, f"d={d} self-check", max_pairs=33 * 200, absent=())
        vec.set_option("check_brackets", 0)
        assert vec.bound_violations() - v0 == 0 and vec.bound_checked() - c0 == known


@pytest.mark.parametrize("d", [12, 513])
def test_dimensions_outside_the_bracket_take_todays_kernels(d):
    from freddy_amd import gpu
    ids, x = si.table(d, 300)
    vec = gpu.VectorIndex(ids, x)
    a, b = ids[:20], ids[100:170]
    check(vec, ids, x, a, b, threshold(ids, x, a, b), f"d={d}", mode=1, kernels=(TODAY,), absent=(FILTER,))
    vec.close()


def test_near_duplicates_and_zero_similarities():
    """rows equal up to their last mantissa bits, t inside the cluster; orthogonal rows (the chain is exactly zero) at t = +0.0 and -0.0"""
    from freddy_amd import gpu
    rng = np.random.default_rng(5)
    base = si.table(300)[1][7]
    x = np.tile(base, (400, 1)).view(np.uint32)
    x = (x + rng.integers(0, 4, size=x.shape).astype(np.uint32)).view(np.float32)
    x[300:] = si.table(300)[1][300:400]
    ids = np.arange(1, 401, dtype=np.int32)
    vec = gpu.VectorIndex(ids, x)
    a, b = ids[:40], ids[20:330]
    m = sm.matrix(ids, x, a, b)[0]
    t = np.float32(np.median(m[:, :280]))
    got, _ = check(vec, ids, x, a, b, t, "near-duplicates")
    assert 0 < got[3] < 40 * 280
    vec.close()
    e = np.zeros((40, 16), np.float32)
    e[np.arange(40), np.arange(40) % 16] = np.where(np.arange(40) % 3 == 0, -0.5, 0.75)
    ids = np.arange(1, 41, dtype=np.int32)
    vec = gpu.VectorIndex(ids, e)
    for t in (np.float32(0.0), np.float32(-0.0)):
        got, _ = check(vec, ids, e, ids, ids, t, f"orthogonal rows t={t!r}")
        assert 0 < got[3] < 1600
    vec.close()


@pytest.mark.parametrize("d", [300, 16])
def test_non_finite_rows_huge_and_tiny_rows_and_special_thresholds(d):
    """a non-finite element in A and B rows, rows at 2^60 and 2^-60 (their scale leaves the pass's window): the unfit pairs are answered
    by the chain, the healthy ones unchanged; t = NaN: nothing; +inf: only NaN similarities; -inf: every known pair -- dense, so value 1
    falls back to today's kernels and value 2 does not"""
    from freddy_amd import gpu
    ids, x, rows = si.poisoned_table(d)
    x = x.copy()
    x[10] *= np.float32(2.0 ** 60)
    x[11] *= np.float32(2.0 ** -60)
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(d)
    a = np.concatenate([ids[rows], ids[[10, 11]], si.draw_ids(ids, 25, rng)]).astype(np.int32)
    b = np.concatenate([ids[rows], ids[[10, 11]], si.draw_ids(ids, 190, rng)]).astype(np.int32)
    clean = si.table(d)[1]
    t = threshold(ids, clean, a, b)
    check(vec, ids, x, a, b, t, f"d={d} poisoned")
    check(vec, ids, x, a, b, np.float32(np.nan), "t=NaN")
    got, _ = check(vec, ids, x, a, b, np.float32(np.inf), "t=+inf")
    assert got[3] > 0 and np.isnan(got[2]).all()
    check(vec, ids, x, a, b, np.float32(-np.inf), "t=-inf, value 2")
    check(vec, ids, x, a, b, np.float32(-np.inf), "t=-inf, value 1", mode=1, kernels=(FILTER, TODAY), absent=())
    vec.close()


def test_max_pairs_passes_and_the_fallback_of_one_pass(handles):
    vec, ids, x = handles(300)
    a, b = si.matrix_case(300, 70, 200)
    t = threshold(ids, x, a, b, frac=0.05)
    total = sm.join(ids, x, a, b, t)[3]
    assert total > 5
    for cap in (0, 1, total - 1, total + 5):
        check(vec, ids, x, a, b, t, f"max_pairs={cap}", max_pairs=cap)
    vec.set_option("similarity_pass_bytes", 1)          # 32 rows per filter pass: 32, 32 and 6
    got, names = check(vec, ids, x, a, b, t, "three passes", max_pairs=70 * 200)
    assert names[FILTER][0] == 3 and (got[0] < 32).any() and (got[0] >= 64).any(), names
    # two passes, only the second dense: 32 random directions (no similarity near t), then 32 rows of the clustered table
    g = np.random.default_rng(3).standard_normal((32, 300))
    av = np.concatenate([g / np.linalg.norm(g, axis=1, keepdims=True), x[200:232]]).astype(np.float32)
    m, _, kb = sm.matrix(ids, x, av, b)
    t2 = np.float32(0.35)
    assert (m[:32] < t2 - 0.05).all() and (m[32:][:, kb] > t2).mean() > 1 / 8
    got, names = check(vec, ids, x, av, b, t2, "the second pass falls back", mode=1, max_pairs=64 * 200, kernels=(FILTER, TODAY), absent=())
    assert names[FILTER][0] == 2 and names[TODAY][0] == 2 and (got[0] >= 32).all()
    vec.set_option("similarity_pass_bytes", 0)


def test_after_append_and_remove_a_call_equals_a_fresh_pins():
    from freddy_amd import gpu
    ids0, x0 = si.table(300)
    ids, x = ids0[:2600].copy(), x0[:2600].copy()
    vec = gpu.VectorIndex(ids, x)
    vec.append_rows(ids0[2600:], vectors=x0[2600:])
    gone = ids0[50:350:3]
    vec.remove_rows(gone)
    keep = ~np.isin(ids0, gone)
    ids, x = ids0[keep], x0[keep]
    fresh = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(11)
    a, b = si.draw_ids(ids0, 40, rng), si.draw_ids(ids0, 300, rng)
    t = threshold(ids, x, a, b)
    got, _ = check(vec, ids, x, a, b, t, "the mutated handle")
    same(join(fresh, a, b, t, 2)[0], got, "a fresh pin")
    vec.close()
    fresh.close()
