"""-m gpu tests of freddy_gpu_cluster (csrc/cluster.h): the whole k-means of cluster_exact / cluster_pq in one call, against the numpy
model of tests/cluster_model.py bit for bit -- clusters, similarity bits and centroid bits -- on the 20 000-row tables and the two
shapes of tests/test_gpu_assign.py (300-d with m = 12; 25-d with m = 5, where d % 4 != 0): sizes around a wave, 256 positions and a
pass, the steered cases of tests/cluster_inputs.py, passes and reuse, mutation, refusals, allocation failures, and through the host
mirror."""
import ctypes as C

import numpy as np
import pytest

import cluster_inputs as ci
import cluster_model as cm

pytestmark = pytest.mark.gpu

N = ci.N
E_ARG, E_NOMEM, E_KIND, E_LIMIT = -1, -3, -4, -5


@pytest.fixture(scope="module", params=list(ci.SHAPES))
def tabs(request):
    from freddy_amd import gpu
    x, ids, cb, codes = ci.tables(request.param)
    vec = gpu.VectorIndex(ids, x)
    pq = gpu.PQIndex(cb, ids, codes)
    rng = np.random.default_rng(19)
    tokens = rng.choice(ids, 1000).astype(np.int32)                    # unsorted, with repeats
    tokens[3] = tokens[1]; tokens[64] = tokens[63]
    tokens[10:20] = np.arange(101, 111); tokens[20:30] = np.arange(5001, 5011)      # duplicated rows
    yield dict(x=x, ids=ids, cb=cb, codes=codes, vec=vec, pq=pq, tokens=tokens, shape=request.param, draws=rng.random(cm.n_draws(100, 10)))
    vec.close(); pq.close()


def _model(t, oracle, method, tokens, kc, draws, rounds, sentinel=1000.0, x=None, ids=None):
    x, ids = (t["x"], t["ids"]) if x is None else (x, ids)
    if method == "exact":
        return cm.exact(ids, x, tokens, kc, draws, rounds)
    return cm.pq(oracle, ids, x, t["cb"], t["ids"], t["codes"], tokens, kc, draws, rounds, sentinel=sentinel)


def _device(t, method, tokens, kc, draws, rounds, sentinel=1000.0, vec=None):
    return (vec or t["vec"]).cluster(tokens, kc, draws, rounds=rounds, pq=t["pq"] if method == "pq" else None, sentinel=sentinel)


def _check(t, oracle, method, tokens, kc, draws, rounds, what, sentinel=1000.0):
    exp = _model(t, oracle, method, tokens, kc, draws, rounds, sentinel)
    got = _device(t, method, tokens, kc, draws, rounds, sentinel)
    assert cm.same(got, exp), f"{what}: clusters differ at {np.flatnonzero(got[0] != exp['clusters'])[:8]}"
    return got, exp


# ---- against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["exact", "pq"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_around_a_wave_and_256_positions(tabs, oracle, method, n):
    t = tabs
    _check(t, oracle, method, t["tokens"][:n], 5, t["draws"][:cm.n_draws(5, 2)], 2, f"{method} n={n}")


@pytest.mark.parametrize("method", ["exact", "pq"])
@pytest.mark.parametrize("kc", [1, 17, 100])
def test_ten_rounds(tabs, oracle, method, kc):
    """kc = 1, one past the exact kernel's tile of 16 queries, and 100 -- as the assign tests."""
    t = tabs
    got, _ = _check(t, oracle, method, t["tokens"], kc, t["draws"][:cm.n_draws(kc, 10)], 10, f"{method} kc={kc}")
    assert got[0].min() >= 1 and got[0].max() <= kc


@pytest.mark.parametrize("method", ["exact", "pq"])
def test_one_round(tabs, oracle, method):
    """rounds = 1: the initial centroids come back, and kc draws are enough."""
    t = tabs
    got, _ = _check(t, oracle, method, t["tokens"][:300], 7, t["draws"][:7], 1, method)
    first = np.array([cm.pick(300, r) - 1 for r in t["draws"][:7]])
    assert np.array_equal(got[2].view(np.uint32), t["x"][t["tokens"][:300][first] - 1].view(np.uint32))


def test_steered_cases(oracle):
    """tests/cluster_inputs.py (built on the 25-d tables): ranks 1 and len, sampled members on both sides of a wave, of 256 positions and
    of a step of the walk, a member drawn twice, an empty cluster in front of sampling ones, stale members, positions that end in
    cluster 0, kc > n, kc = 1."""
    from freddy_amd import gpu
    x, ids, cb, codes = ci.tables("25d_m5")
    t = dict(x=x, ids=ids, cb=cb, codes=codes, vec=gpu.VectorIndex(ids, x), pq=gpu.PQIndex(cb, ids, codes))
    for walk in (2, 1):                     # the two-level walk over the apply kernel's counts, and the plain walk from position 0
        t["vec"].set_option("cluster_walk", walk)
        for case in ci.steered_cases():
            got, exp = _check(t, oracle, case["method"], case["tokens"], case["kc"], case["draws"], case["rounds"], f"{case['name']} walk={walk}",
                              case["sentinel"])
            if case["name"] == "unclaimed":
                assert (got[0] == 0).any() and np.isneginf(got[1][got[0] == 0]).all()
    t["vec"].close(); t["pq"].close()


def test_more_clusters_than_a_workgroup_counts(oracle):
    """kc = 1025, one past the 1024 clusters whose lengths and per-block members cluster_apply_kernel counts in LDS: global atomics and
    the plain walk, over more than one step of 2048 positions."""
    from freddy_amd import gpu
    x, ids, _, _ = ci.tables("25d_m5")
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(23)
    tokens = rng.choice(ids, 5000).astype(np.int32)
    draws = rng.random(cm.n_draws(1025, 3))
    exp = cm.exact(ids, x, tokens, 1025, draws, 3)
    got = vec.cluster(tokens, 1025, draws, rounds=3)
    assert cm.same(got, exp), np.flatnonzero(got[0] != exp["clusters"])[:8]
    exp = cm.exact(ids, x, tokens, 1024, draws, 3)
    vec.set_option("cluster_walk", 2)
    assert cm.same(vec.cluster(tokens, 1024, draws, rounds=3), exp)
    vec.close()


def test_the_walk_chosen_from_16_steps_on(oracle):
    """n = 16 * 2048 (the plain walk) and one token more (the two-level walk, chosen by the call itself), kc = 5."""
    from freddy_amd import gpu
    x, ids, _, _ = ci.tables("25d_m5")
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(29)
    tokens = rng.choice(ids, 16 * ci.STEP + 1).astype(np.int32)
    draws = rng.random(cm.n_draws(5, 3))
    for n in (16 * ci.STEP, 16 * ci.STEP + 1):
        exp = cm.exact(ids, x, tokens[:n], 5, draws, 3)
        assert cm.same(vec.cluster(tokens[:n], 5, draws, rounds=3), exp), n
    vec.close()


def test_a_sentinel_that_leaves_tokens_unclaimed(tabs, oracle):
    t = tabs
    sentinel = 0.5 if t["shape"] == "25d_m5" else 0.9
    got, exp = _check(t, oracle, "pq", t["tokens"][:400], 6, t["draws"][:cm.n_draws(6, 4)], 4, "pq, low sentinel", sentinel)
    assert np.isneginf(got[1]).any() and not np.isneginf(got[1]).all()


def test_a_token_row_with_a_nan(tabs, oracle):
    """One token's row holds a NaN: its similarity is a NaN for every centroid (above every number: the first centroid claims it), and
    a centroid that samples it becomes NaN.  The model decides; the device agrees."""
    from freddy_amd import gpu
    t = tabs
    n0 = 2000
    x = t["x"][:n0].copy()
    x[7, 3] = np.nan
    vec = gpu.VectorIndex(t["ids"][:n0], x)
    rng = np.random.default_rng(5)
    tokens = rng.choice(t["ids"][:n0], 200).astype(np.int32)
    tokens[11] = 8; tokens[150] = 8
    draws = rng.random(cm.n_draws(4, 4))
    exp = cm.exact(t["ids"][:n0], x, tokens, 4, draws, 4)
    got = vec.cluster(tokens, 4, draws, rounds=4)
    vec.close()
    assert cm.same(got, exp) and np.isnan(got[1][11]) and np.isnan(got[1][150])


# ---- passes and reuse ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["exact", "pq"])
def test_passes_of_256_targets_and_repeated_calls(tabs, oracle, method):
    t = tabs
    kc, rounds = 9, 3
    draws = t["draws"][:cm.n_draws(kc, rounds)]
    big = _device(t, method, t["tokens"], kc, draws, rounds)
    again = _device(t, method, t["tokens"], kc, draws, rounds)
    t["vec"].set_option("cluster_pass", 256)
    try:
        passes = _device(t, method, t["tokens"], kc, draws, rounds)
        t["vec"].set_option("cluster_walk", 2)
        plain = _device(t, method, t["tokens"], kc, draws, rounds)      # (n = 1000 takes the plain walk by itself: this is the other one)
    finally:
        t["vec"].set_option("cluster_pass", 0)
        t["vec"].set_option("cluster_walk", 0)
    exp = _model(t, oracle, method, t["tokens"], kc, draws, rounds)
    assert cm.same(big, exp) and cm.same(again, exp) and cm.same(passes, exp) and cm.same(plain, exp)
    _check(t, oracle, method, t["tokens"][:70], 3, draws[:cm.n_draws(3, 3)], 3, "a small call after a large one")


# ---- mutation --------------------------------------------------------------------------------------------------------------------------
def test_a_call_sees_append_remove_and_update(tabs):
    """After append_rows, remove_rows and update_rows on the vector handle the call equals that of a fresh pin of the same table."""
    from freddy_amd import gpu
    t = tabs
    cut = N - 500
    rng = np.random.default_rng(11)
    x = t["x"].copy()
    vec = gpu.VectorIndex(t["ids"][:cut], x[:cut])
    vec.append_rows(t["ids"][cut:], vectors=x[cut:])
    gone = rng.choice(t["ids"], 300, replace=False).astype(np.int32)
    vec.remove_rows(gone)
    keep = np.setdiff1d(t["ids"], gone)
    changed = rng.choice(keep, 200, replace=False).astype(np.int32)
    x[changed - 1] = x[rng.choice(N, 200)]
    vec.update_rows(changed, vectors=x[changed - 1])
    fresh = gpu.VectorIndex(keep, x[keep - 1])
    tokens = np.concatenate([rng.choice(keep, 500), changed[:50], np.arange(cut + 1, cut + 51)]).astype(np.int32)
    tokens = tokens[np.isin(tokens, keep)]
    draws = rng.random(cm.n_draws(6, 4))
    a, b = vec.cluster(tokens, 6, draws, rounds=4), fresh.cluster(tokens, 6, draws, rounds=4)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))
    with pytest.raises(gpu.FreddyGpuError, match=f"token id {int(gone[0])} has no vector"):
        vec.cluster(np.concatenate([tokens[:5], gone[:1]]).astype(np.int32), 2, draws, rounds=2)
    vec.close(); fresh.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(tabs):
    from freddy_amd import gpu
    t = tabs
    lib, vec, pq = t["vec"].lib, t["vec"], t["pq"]
    d = t["x"].shape[1]
    n, kc, rounds = 100, 4, 3
    tok = np.ascontiguousarray(t["tokens"][:n])
    draws = np.ascontiguousarray(t["draws"][:cm.n_draws(kc, rounds)])
    oc = np.full(n, -7, np.int32); osim = np.full(n, 3.5, np.float32); ocent = np.full((kc, d), 2.5, np.float32)
    P = gpu._p
    err = lambda: lib.freddy_gpu_last_error().decode()      # noqa: E731

    def call(vecs=vec.h, pqh=None, sentinel=1000.0, tokens=tok, n=n, kc=kc, rounds=rounds, dr=draws, n_draws=None, out=oc):
        return lib.freddy_gpu_cluster(vecs, pqh, C.c_float(sentinel), None if tokens is None else P(tokens), n, kc, rounds,
                                      None if dr is None else P(dr), n_draws if n_draws is not None else (0 if dr is None else dr.size),
                                      None if out is None else P(out), P(osim), P(ocent))

    nan_draw = draws.copy(); nan_draw[kc + 3] = np.nan
    unknown = tok.copy(); unknown[40] = N + 9; unknown[77] = -3
    other_d = gpu.VectorIndex(np.arange(1, 65, dtype=np.int32), np.zeros((64, d + 1), np.float32))
    fake = C.c_void_p(8)          # a handle that is never looked at: the scalars are refused before that
    refused = [
        (lambda: call(vecs=fake, n=0), E_ARG, "n=0"), (lambda: call(vecs=fake, kc=0), E_ARG, "kc=0"), (lambda: call(vecs=fake, rounds=0), E_ARG, "rounds=0"),
        (lambda: call(vecs=fake, tokens=None), E_ARG, "NULL buffer"), (lambda: call(vecs=fake, dr=None), E_ARG, "NULL buffer"),
        (lambda: call(vecs=fake, out=None), E_ARG, "NULL buffer"),
        (lambda: call(vecs=fake, n_draws=cm.n_draws(kc, rounds) - 1), E_ARG, f"n_draws={cm.n_draws(kc, rounds) - 1}"),
        (lambda: call(vecs=fake, dr=nan_draw), E_ARG, f"draw {kc + 3} is not a number"),
        (lambda: call(vecs=fake, pqh=fake, sentinel=float("nan")), E_ARG, "sentinel"), (lambda: call(vecs=fake, pqh=fake, sentinel=16777217.0 * 2), E_ARG, "sentinel"),
        (lambda: call(vecs=fake, kc=65537, n_draws=10 ** 9), E_LIMIT, "kc=65537"), (lambda: call(vecs=fake, n=2 ** 31), E_LIMIT, f"n={2 ** 31}"),
        (lambda: call(vecs=None), E_ARG, "NULL index"),
        (lambda: call(vecs=pq.h), E_KIND, "wrong kind"), (lambda: call(pqh=vec.h), E_KIND, "wrong kind"),
        (lambda: call(vecs=other_d.h, pqh=pq.h), E_ARG, "different dimensions"),
        (lambda: call(tokens=unknown), E_ARG, f"token id {N + 9} has no vector"),
        (lambda: call(pqh=pq.h, tokens=unknown), E_ARG, f"token id {N + 9} has no vector"),
    ]
    for i, (fn, code, text) in enumerate(refused):
        rc = fn()
        assert rc == code and text in err(), (i, rc, err())
        assert (oc == -7).all() and (osim == 3.5).all() and (ocent == 2.5).all(), f"refusal {i} wrote an output"
    assert call(vecs=fake, n_draws=3) == E_ARG
    assert "n_draws=3" in err() and str(cm.n_draws(kc, rounds)) in err()      # both numbers
    other_d.close()
    # a NaN beyond the draws the call uses is not looked at; out_sim and out_centroids may be NULL
    longer = np.concatenate([draws, [np.nan]])
    assert lib.freddy_gpu_cluster(vec.h, None, C.c_float(0), P(tok), n, kc, rounds, P(longer), longer.size, P(oc), None, None) == 0
    assert np.array_equal(oc, vec.cluster(tok, kc, draws, rounds=rounds)[0]) and (osim == 3.5).all()


# ---- allocation failures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["exact", "pq"])
def test_every_allocation_fails_once(tabs, oracle, method):
    """FLOORS (cluster.hip freddy_gpu_cluster): ids, rows, clusters, best, sim, centroids, lens + flag, draws, per-block members = 9; pq: +
    the smallest distances and the LUTs = 11 (and what launch_lut needs)."""
    from freddy_amd import gpu
    t = tabs
    n0 = 1500
    ids, x = t["ids"][:n0], t["x"][:n0]
    rng = np.random.default_rng(13)
    tokens = rng.choice(ids, 130).astype(np.int32)
    kc, rounds = 4, 3
    draws = rng.random(cm.n_draws(kc, rounds))
    pq = gpu.PQIndex(t["cb"], ids, t["codes"][:n0]) if method == "pq" else None
    exp = cm.exact(ids, x, tokens, kc, draws, rounds) if method == "exact" else \
        cm.pq(oracle, ids, x, t["cb"], ids, t["codes"][:n0], tokens, kc, draws, rounds)
    def call(v, p):          # (the two-level walk, which 130 tokens would not take by themselves: its block counts are an allocation too)
        v.set_option("cluster_walk", 2)
        return v.cluster(tokens, kc, draws, rounds=rounds, pq=p)

    gpu.alloc_fail_nth(0)
    vec = gpu.VectorIndex(ids, x)
    c0 = gpu.alloc_stats().calls
    got = call(vec, pq)
    A = gpu.alloc_stats().calls - c0
    vec.close()
    assert cm.same(got, exp)
    assert A >= (9 if method == "exact" else 11), A
    for k in range(1, A + 1):
        what = f"{method} k={k}/{A}"
        vec = gpu.VectorIndex(ids, x)
        if pq is not None:
            pq.close()
            pq = gpu.PQIndex(t["cb"], ids, t["codes"][:n0])
        failed0 = gpu.alloc_stats().failed
        gpu.alloc_fail_nth(k)
        err = None
        try:
            call(vec, pq)
        except gpu.FreddyGpuError as e:
            err = e
        finally:
            gpu.alloc_fail_nth(0)
        assert err is not None and err.code == gpu.E_NOMEM, f"{what}: {err}"
        assert gpu.alloc_stats().failed - failed0 == 1, what
        oi, od, q = np.empty((1, 1), np.int32), np.empty((1, 1), np.float32), np.zeros((1, x.shape[1]), np.float32)
        assert vec.lib.freddy_gpu_exact_search(vec.h, gpu._p(q), 1, 0, None, 0, gpu._p(oi), gpu._p(od)) == E_ARG, f"{what}: the handle is poisoned"
        assert cm.same(call(vec, pq), exp), f"{what}: the call made again differs from the model"
        vec.close()
    if pq is not None:
        pq.close()


# ---- through the host mirror --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["exact", "pq"])
def test_host_mirror_runs_the_one_call(oracle, which):
    """cluster_exact / cluster_pq at n = 5000: the profile of the vector handle names the kernels of csrc/cluster.h, the result is the
    model's, and a call with part of the draws supplied continues with the mirror's own generator; exact_assign names none of them."""
    from freddy_amd import udf
    import util
    x = util.corpus(N).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    pq = util.pq_tables(N=N, K=256)
    s = udf.Session()
    s.load_vecs_norm(ids, x)
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    rng = np.random.default_rng(43)
    n, k = 5000, 3
    tokens = rng.choice(ids, n).astype(np.int32)
    draws = rng.random(cm.n_draws(k, 10))
    s.exact_assign(x[:1], tokens[:1])                 # (pins the vectors: the handle exists before it is profiled)
    idx = s.gpu_index("vecs")
    idx.profile_enable(True)
    s.exact_assign(x[:2], tokens[:100])
    names = set(idx.profile_read())
    assert "assign_exact_kernel" in names and not [m for m in names if m.startswith("cluster_")], names
    idx.profile_enable(True)
    got = getattr(s, "cluster_" + which)(tokens, k, draws)
    names = set(idx.profile_read())
    idx.profile_enable(False)
    assert {"cluster_init_kernel", "cluster_apply_kernel", "cluster_sample_kernel"} <= names, names
    exp = cm.exact(ids, x, tokens, k, draws, 10) if which == "exact" else \
        cm.pq(oracle, ids, x, pq["codebook"], pq["ids"], pq["codes"], tokens, k, draws, 10)
    assert np.array_equal(got, exp["clusters"])
    # the first 7 draws supplied: the mirror's xorshift gives the others (host/cluster.h)
    state, own = 0x9E3779B97F4A7C15, []
    for _ in range(cm.n_draws(k, 10) - 7):
        state ^= (state << 13) & (2 ** 64 - 1); state ^= state >> 7; state ^= (state << 17) & (2 ** 64 - 1)
        own.append((state >> 11) / 9007199254740992.0)
    mixed = np.concatenate([draws[:7], own])
    exp = cm.exact(ids, x, tokens[:500], k, mixed, 10) if which == "exact" else \
        cm.pq(oracle, ids, x, pq["codebook"], pq["ids"], pq["codes"], tokens[:500], k, mixed, 10)
    assert np.array_equal(getattr(s, "cluster_" + which)(tokens[:500], k, draws[:7]), exp["clusters"])
    s.close()
