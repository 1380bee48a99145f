"""-m gpu: option assign_filter (csrc/assign_filter.h, the asf_* host code of csrc/cluster.hip) where tests/test_gpu_assign_filter.py
stops: a bracket under pressure (near-ties of 0 .. 6 eps, wide dynamic range, cancellation, all-negative similarities against the
zero padding, zero vectors, the scale exponents at +-ENC_MAX_EXP), the candidate lists over three and more tiles, the redo kernel's
partial workgroups, the passes of freddy_gpu_exact_assign, whole k-means with redos inside them, and the handle's state.

Every result is compared bit for bit with assign_model.exact_assign (the k-means: with the same call, option off).  The inputs and
predicted_redo() come from tests/assign_filter_inputs.py; tests/test_assign_filter_inputs_cpu.py proves there what is assumed here:
st["redone"] is asserted EXACTLY, st["filtered"] is the number of targets with a row."""
import numpy as np
import pytest

import assign_filter_inputs as fi
import assign_model as am
import util

pytestmark = pytest.mark.gpu


def filtered_vec(ids, x, check=False):
    from freddy_amd import gpu
    vec = gpu.VectorIndex(ids, x)
    vec.set_option("assign_filter", 1)
    if check:
        vec.set_option("check_brackets", 16)
    return vec


def run(vec, x, ids, qs, tg, redone, what, exp=None):
    """assign == the model, filtered == targets with a row, redone == the prediction (an int, or None: predicted_redo of the inputs)."""
    got = vec.assign(qs, tg)
    exp = am.exact_assign(ids, x, qs, tg) if exp is None else exp
    assert am.same(got, exp), f"{what}: {np.flatnonzero(got[0] != exp[0])[:8]}"
    st = vec.last_assign_stats()
    have, rows = fi.target_rows(ids, x, tg)
    if redone is None:
        redone = int(fi.predicted_redo(rows, qs).sum())
    assert st["filtered"] == have.sum() and st["redone"] == redone, (what, st, redone)
    return got, st, int(have.sum())


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("d", fi.DIMS)
def test_near_ties(d, wide):
    """assign_filter_kernel's MFMA loop and fragment layouts (the six products per k-step, asf_load8, the image's lane order) and
    the filter's comparisons: groups of six centroids 0 .. 6 eps below a probe target's best, in both tiles of Q = 200 -- a wrong operand
    in one k-step or a dropped lo.hi product moves a by more than these gaps and fails here (winner or `violations`).  What this does
    NOT detect is an asf_eps_rel that is merely too small: the filter's real error on these inputs is far below the bracket (the
    header's bound is a worst case times 3.1), so half the constant still holds every bracket and keeps every winner.
    wide: elements spanning 2^-12 .. 1, lo halves subnormal in f16 (the header's 2^-38 term)."""
    x, ids, qs, tg, probes, groups = fi.near_ties(d, wide)
    vec = filtered_vec(ids, x)
    got, st, n_rows = run(vec, x, ids, qs, tg, 0, f"near ties d={d}")
    assert np.isin(got[0][probes], groups).all()            # (tg[i] = ids[i]: position = row)
    vec.set_option("check_brackets", 16)
    got, st, _ = run(vec, x, ids, qs, tg, 0, f"near ties d={d}, self-check")
    assert st["violations"] == 0 and st["checked"] == n_rows * fi.Q_TIES, st
    vec.close()


@pytest.mark.parametrize("d", fi.DIMS)
def test_cancellation(d):
    """The bracket's P = sum |x_j q_j| term (header, "reference chain" and "MFMA accumulation"): similarities within a few eps of 0 with
    both signs while P ~ |x||q| -- the chain's and the matrix core's rounding errors are as large against the result as they get."""
    x, ids, qs, tg = fi.cancellation(d)
    vec = filtered_vec(ids, x, check=True)
    got, st, n_rows = run(vec, x, ids, qs, tg, 0, f"cancellation d={d}")
    assert st["violations"] == 0 and st["checked"] == n_rows * qs.shape[0], st
    vec.close()


@pytest.mark.parametrize("Q", [1, 127, 129, 257])
def test_all_negative_similarities_against_the_padding(Q):
    """The epilogue's `valid` test (assign_filter_kernel, `cbase + ... < a.Q`): the zero centroids that pad Q to 128 have a = 0, above
    every real similarity here."""
    x, ids, qs, tg = fi.all_negative(30, Q)
    vec = filtered_vec(ids, x)
    got, st, _ = run(vec, x, ids, qs, tg, None, f"all negative Q={Q}")
    assert st["redone"] == 0
    have = am.rows_of(ids, tg) >= 0
    assert (got[0][have] >= 0).all() and (got[0][~have] == -1).all()
    vec.close()


def test_zero_rows_and_zero_centroids():
    """Steps b / c with a = 0 everywhere (eps = ENC_EPS_ABS alone, L = -eps): a zero row keeps 16 ties and is redone at 17; a zero
    centroid among ordinary ones; an all-zero set (max|q| = 0, ec = 0 in assign_image_kernel's phase 1)."""
    for name, (x, ids, qs, tg, winner) in fi.zero_cases().items():
        vec = filtered_vec(ids, x)
        got, st, _ = run(vec, x, ids, qs, tg, {"zero_row_Q17": 1, "zero_centroid": 1}.get(name, 0), name)
        assert got[0][0 if name != "all_zero_centroids" else 3] == winner, name
        vec.close()


def test_scale_exponents_at_the_edges():
    """scale_ok in assign_filter_kernel (e, e + ecp against +-ENC_MAX_EXP) and the image's flag for ec (assign_image_kernel, phase 1):
    a row out of range redoes that target only, a centroid scale out of range every target, a sum out of range that target.  Then a
    healthy call on the same handle."""
    rng = np.random.default_rng(1)
    for name, (x, ids, qs, tg) in fi.scale_cases().items():
        vec = filtered_vec(ids, x)
        run(vec, x, ids, qs, tg, int(fi.scale_redo(x[tg - 1], qs).sum()), name)
        hq = rng.standard_normal(qs.shape).astype(np.float32)
        hx = rng.standard_normal((5, x.shape[1])).astype(np.float32)
        vec.update_rows(ids[:5], vectors=hx)                                    # (the scaled rows of the case live in rows 0 .. 4)
        x2 = x.copy(); x2[:5] = hx
        run(vec, x2, ids, hq, tg, 0, name + ", then healthy")
        vec.close()


@pytest.mark.parametrize("Q", fi.B_QS)
def test_lists_over_three_and_more_tiles(Q):
    """Steps b and c of assign_filter_kernel over nit >= 3 tiles (the prefetch of the next tile's operands, lists carried over
    boundaries), the final filter + sort, and assign_redo_kernel's partial workgroups (`slot < count`, `blockIdx.x * 64 >= count`):
    plateaus of exact copies -- 16 kept / 17 redone in tile 0 and in the last tile, spread over tiles, a compaction that succeeds
    (`if (av + eps >= Lrow)` shrinks a list above ENC_KEEP), exactly ENC_CAP entries, 33 arrivals, redo lists of 63 / 64 / 65 / 128."""
    vec = None
    for name, (x, ids, qs, tg, pos, winner, redone) in fi.list_cases(Q).items():
        vec = vec or filtered_vec(ids, x)
        got, st, _ = run(vec, x, ids, qs, tg, None, f"Q={Q} {name}")
        assert st["redone"] == (len(pos) if redone else 0) and np.array_equal(got[0][pos], winner), name
    vec.close()


def test_second_pass_of_exact_assign():
    """freddy_gpu_exact_assign's pass loop with the option on: n = AS_PASS + 65 -- asf_pass's `if (!first_pass) assign_begin_kernel(head,
    0, 0)` (redo_cnt of the second pass starts at 0, the counters go on), buffers carved for AS_PASS targets."""
    n = fi.AS_PASS + 65
    x, ids, qs, tg = fi.pass_case(n, 100, 3, fi.AS_PASS)
    vec = filtered_vec(ids, x)
    run(vec, x, ids, qs, tg, 103, "two passes", exp=fi.model_by_id(ids, x, qs, tg))
    vec.close()


def test_second_pass_under_the_self_check():
    """asf_check_pass: Qpad = 128 gives passes of 2^20 targets under check_brackets = 16; n = 2^20 + 65 is two of them.  A redone target
    is not refined (assign_refine_kernel: n_ref = 0 for cnt < 0), so checked = (filtered - redone) Q."""
    first = fi.check_pass(17)
    n = first + 65
    x, ids, qs, tg = fi.pass_case(n, 100, 3, first)
    vec = filtered_vec(ids, x, check=True)
    got, st, n_rows = run(vec, x, ids, qs, tg, 103, "two passes, self-check", exp=fi.model_by_id(ids, x, qs, tg))
    assert st["violations"] == 0 and st["checked"] == (n_rows - 103) * 17, st
    vec.close()


def test_self_check_with_a_redo():
    """check_brackets = 16 with a redo in the call: the redone targets leave `checked`, every other bracket holds."""
    name, (x, ids, qs, tg, pos, winner, redone) = "17_in_tile0", fi.list_cases(300)["17_in_tile0"]
    vec = filtered_vec(ids, x, check=True)
    got, st, n_rows = run(vec, x, ids, qs, tg, len(pos), name)
    assert st["violations"] == 0 and st["checked"] == (n_rows - len(pos)) * 300, st
    vec.close()


# =======================================================================================
# whole k-means, option on against option off
# =======================================================================================
def same3(on, off):
    ok = np.array_equal(on[0], off[0])
    for g, e in ((on[1], off[1]), (on[2], off[2])):
        nan = np.isnan(e)
        ok = ok and np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.uint32), e[~nan].view(np.uint32))
    return ok


def on_and_off(ids, x, tokens, kc, draws, rounds=10, options=()):
    from freddy_amd import gpu
    vec = gpu.VectorIndex(ids, x)
    for o in options:
        vec.set_option(*o)
    off = vec.cluster(tokens, kc, draws, rounds=rounds)
    vec.set_option("assign_filter", 1)
    vec.profile_enable(True)
    on = vec.cluster(tokens, kc, draws, rounds=rounds)
    names, st = set(vec.profile_read()), vec.last_assign_stats()
    vec.close()
    assert same3(on, off), (kc, rounds, options)
    assert "assign_filter_kernel" in names and "assign_exact_kernel" not in names, names
    return st


@pytest.mark.parametrize("kc,rounds,option", [(129, 10, None), (300, 10, None), (129, 10, ("cluster_pass", 64)), (300, 10, ("cluster_pass", 64)), (300, 1, None)])
def test_kmeans_over_two_and_three_tiles(kc, rounds, option):
    """freddy_gpu_cluster's rounds with kc > 128: asf_image per round, asf_pass per pass; stats summed over the rounds."""
    x = util.corpus(8000).numpy()
    ids = np.arange(1, 8001, dtype=np.int32)
    rng = np.random.default_rng(kc)
    tokens = np.sort(rng.choice(ids, 3000, replace=False)).astype(np.int32)
    st = on_and_off(ids, x, tokens, kc, rng.random(kc + 9 * kc * 10), rounds, [option] if option else [])
    assert st["filtered"] == rounds * 3000, st


def test_kmeans_with_redos_inside():
    """Rows of three distinct vectors, kc = 40: more than 16 identical centroids -- assign_redo_kernel inside the rounds."""
    x, ids, tokens, kc, draws = fi.three_vector_tokens()
    st = on_and_off(ids, x, tokens, kc, draws)
    assert st["redone"] > 0 and st["filtered"] == 10 * tokens.size, st


@pytest.mark.parametrize("check", [False, True])
def test_kmeans_with_non_finite_rows(check):
    """The image's flag recomputed per round (asf_image, assign_begin_kernel(head, 1, ...)): rows with NaN / +-Inf are redone in round
    one, a round whose sampled centroid is non-finite redoes every target, a later round with finite centroids filters again."""
    x, ids, tokens, kc, draws = fi.nan_tokens(fi.NAN_SEED)
    n = tokens.size
    st = on_and_off(ids, x, tokens, kc, draws, options=[("check_brackets", 16), ("cluster_pass", 64)] if check else [])
    assert st["filtered"] == 10 * n and n <= st["redone"] < 10 * n, st
    if check:
        assert st["violations"] == 0 and st["checked"] > 0, st


def test_one_handle_through_shrinking_and_growing_centroid_sets():
    """asf_img / asf_work reused across calls (DevBuf::ensure in asf_begin keeps the larger buffer): cluster(kc = 300), assign(Q = 5),
    assign(Q = 300), cluster(kc = 7) on one handle."""
    from freddy_amd import gpu
    x = util.corpus(8000).numpy()[:2000]
    ids = np.arange(1, 2001, dtype=np.int32)
    rng = np.random.default_rng(8)
    tokens = np.sort(rng.choice(ids, 900, replace=False)).astype(np.int32)
    d300, d7 = rng.random(300 + 9 * 300 * 10), rng.random(7 + 9 * 7 * 10)
    ref = gpu.VectorIndex(ids, x)
    off300, off7 = ref.cluster(tokens, 300, d300), ref.cluster(tokens, 7, d7)
    ref.close()
    vec = filtered_vec(ids, x)
    assert same3(vec.cluster(tokens, 300, d300), off300)
    qs = np.stack([x[rng.choice(2000, 10)].mean(axis=0) for _ in range(300)]).astype(np.float32)
    tg = np.concatenate([tokens[:200], [5000]]).astype(np.int32)
    for Q in (5, 300):
        assert am.same(vec.assign(qs[:Q], tg), am.exact_assign(ids, x, qs[:Q], tg)), Q
        assert vec.last_assign_stats()["filtered"] == 200
    assert same3(vec.cluster(tokens, 7, d7), off7)
    assert vec.last_assign_stats()["filtered"] == 10 * 900
    vec.close()


# =======================================================================================
# mutations and the pin-time switch
# =======================================================================================
def test_after_update_append_remove():
    """The filter reads ix->coarse / ix->ids / ix->N of the mutated table (AsfFilterArgs in asf_pass): after update_rows, append_rows and
    remove_rows, assign equals the model on the mutated table and a fresh pin."""
    x, ids, qs, tg, probes, groups = fi.near_ties(65)
    x, ids = x.copy(), ids.copy()
    vec = filtered_vec(ids, x)
    spare = np.setdiff1d(np.arange(len(x)), probes)[:2]

    def check(what, redone=0):
        got, _, _ = run(vec, x, ids, qs, tg, redone, what)
        fresh = filtered_vec(ids, x)
        assert am.same(fresh.assign(qs, tg), got), what
        fresh.close()
    x[spare[0]] = x[probes[0]]                                                  # a row becomes a near-tie probe
    x[spare[1], 9] = np.nan
    vec.update_rows(ids[spare], vectors=x[spare])
    check("update_rows", 1)
    x[spare[1]] = x[probes[1]]                                                  # finite again
    vec.update_rows(ids[spare[1:]], vectors=x[spare[1:]])
    check("update_rows back")
    new = (x[:70] * np.float32(0.5)).astype(np.float32)
    new_ids = np.arange(len(x) + 1, len(x) + 71, dtype=np.int32)
    vec.append_rows(new_ids, vectors=new)
    x, ids = np.concatenate([x, new]), np.concatenate([ids, new_ids])
    tg = np.concatenate([tg, new_ids]).astype(np.int32)
    check("append_rows")
    for gone in (ids[10:40], ids[100:170]):                                     # below and above a workgroup's 64 targets
        vec.remove_rows(gone)
        keep = ~np.isin(ids, gone)
        x, ids = x[keep], ids[keep]
        check(f"remove_rows of {gone.size}")
    vec.close()


def test_the_option_from_the_environment(monkeypatch):
    """tune defaults (core.hip: env_int("FREDDY_GPU_ASSIGN_FILTER")) are read at pin time."""
    from freddy_amd import gpu
    name, (x, ids, qs, tg, pos, winner, redone) = "16_in_tile0", fi.list_cases(257)["16_in_tile0"]
    exp = am.exact_assign(ids, x, qs, tg)
    for value, kernel, other in (("1", "assign_filter_kernel", "assign_exact_kernel"), (None, "assign_exact_kernel", "assign_filter_kernel")):
        if value is None:
            monkeypatch.delenv("FREDDY_GPU_ASSIGN_FILTER", raising=False)
        else:
            monkeypatch.setenv("FREDDY_GPU_ASSIGN_FILTER", value)
        vec = gpu.VectorIndex(ids, x)
        vec.profile_enable(True)
        assert am.same(vec.assign(qs, tg), exp)
        names = set(vec.profile_read())
        assert kernel in names and other not in names, (value, names)
        vec.close()
