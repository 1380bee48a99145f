"""-m gpu tests of the assignment step of cluster_exact / cluster_pq (csrc/assign.h): freddy_gpu_exact_assign / freddy_gpu_pq_assign
against the numpy model of tests/assign_model.py bit for bit, against the list-based path they replace (freddy_gpu_exact_join /
freddy_gpu_pq_search at k = n reduced per token on the host), with non-finite queries, rows and codewords, after append_rows, and
through the host mirror: cluster_exact / cluster_pq over 5000 tokens (refused with FREDDY_E_LIMIT before), the kernels' names in
the profile."""
import numpy as np
import pytest

import assign_model as am
import util

pytestmark = pytest.mark.gpu

N = 20000
AS_QT, AS_MAX_Q = 16, 65536           # csrc/dot_chain.h TILE_QT: the exact kernel's query tile; csrc/assign.h AS_MAX_Q: the calls' query limit
SHAPES = {"300d_m12": (300, 12, 256), "25d_m5": (25, 5, 256)}


def _tables(shape):
    d, m, K = SHAPES[shape]
    if d == 300:
        x = util.corpus(N).numpy().copy()
        pq = util.pq_tables(N=N, K=K)
    else:
        x = util.shape_corpus(N, d).numpy().copy()
        pq = util.shape_pq_tables(d, m, K, N)
    codes = pq["codes"].copy()
    x[5000:5040] = x[100:140]             # duplicated rows, in both tables
    codes[5000:5040] = codes[100:140]
    return x, np.arange(1, N + 1, dtype=np.int32), pq["codebook"], codes


@pytest.fixture(scope="module", params=list(SHAPES))
def tabs(request):
    from freddy_amd import gpu
    x, ids, cb, codes = _tables(request.param)
    vec = gpu.VectorIndex(ids, x)
    pq = gpu.PQIndex(cb, ids, codes)
    rng = np.random.default_rng(17)
    cent = np.stack([x[rng.choice(N, 10)].mean(axis=0) for _ in range(100)]).astype(np.float32)   # means of rows, not rows
    cent[4] = cent[0]; cent[16] = cent[3]; cent[40] = cent[39]                                     # identical queries
    targets = rng.choice(ids, 1000).astype(np.int32)
    targets[3] = targets[1]; targets[64] = targets[63]                                             # duplicated ids
    targets[5] = N + 7; targets[62] = -4; targets[700] = 2**31 - 1                                 # ids without a row
    targets[10:20] = np.arange(101, 111); targets[20:30] = np.arange(5001, 5011)                   # duplicated rows
    yield dict(x=x, ids=ids, cb=cb, codes=codes, vec=vec, pq=pq, cent=cent, targets=targets, shape=request.param)
    vec.close(); pq.close()


# ---- against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_assign_equals_the_model(tabs, oracle, n):
    """Q = 1, 5, 17 (one past the exact kernel's tile of 16, and more LUTs than the five or eight one LDS stage holds), 100."""
    t = tabs
    tg = t["targets"][:n]
    for Q in (1, 5, AS_QT + 1, 100):
        qs = t["cent"][:Q]
        got, exp = t["vec"].assign(qs, tg), am.exact_assign(t["ids"], t["x"], qs, tg)
        assert am.same(got, exp), f"exact n={n} Q={Q}: {np.flatnonzero(got[0] != exp[0])[:8]}"
        got, exp = t["pq"].assign(qs, tg), am.pq_assign(oracle, t["cb"], t["ids"], t["codes"], qs, tg)
        assert am.same(got, exp), f"pq n={n} Q={Q}: {np.flatnonzero(got[0] != exp[0])[:8]}"
    if n == 1000:
        q, s = t["vec"].assign(t["cent"], tg)
        assert q[5] == -1 and q[62] == -1 and q[700] == -1 and np.isneginf(s[[5, 62, 700]]).all()
        assert q[3] == q[1] and q[64] == q[63] and np.array_equal(q[10:20], q[20:30])
        assert not np.isin(q, [4, 16, 40]).any(), "the later of two identical queries won a target"
        assert (np.delete(q, [5, 62, 700]) >= 0).all()


@pytest.mark.parametrize("d", [7, 30, 32, 33])
def test_exact_assign_at_the_edges_of_a_step(d):
    """The exact kernel's tiles take 32 dimensions per step: d = 7 (less than one step, odd: the scalar loads), 30 (rows aligned to 8
    bytes, not 16: the scalar loads again), 32 (one full step and no tail) and 33 (a tail of one dimension); 300 rows, 17 queries (a
    tile of 16 and one of one), 65 targets (two waves), some without a row."""
    from freddy_amd import gpu
    n0 = 300
    x = util.shape_corpus(n0, d).numpy()
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    vec = gpu.VectorIndex(ids, x)
    rng = np.random.default_rng(31 + d)
    qs = np.stack([x[rng.choice(n0, 5)].mean(axis=0) for _ in range(AS_QT + 1)]).astype(np.float32)
    tg = rng.choice(ids, 65).astype(np.int32)
    tg[4] = n0 + 9; tg[63] = -2; tg[64] = tg[0]
    for n in (1, 65):
        got, exp = vec.assign(qs, tg[:n]), am.exact_assign(ids, x, qs, tg[:n])
        assert am.same(got, exp), f"d={d} n={n}: {np.flatnonzero(got[0] != exp[0])[:8]}"
    vec.close()


def test_assign_at_the_query_limit(oracle):
    """Q = 65536 on a 2000-row table of the 25-d shape (the model of 65536 wide queries would take too long): 4096 query tiles of the
    exact kernel, and more LUTs (320 MiB) than the 64 MiB built at once -- five chunks, the best carried between the launches."""
    from freddy_amd import gpu
    n0, (d, m, K) = 2000, SHAPES["25d_m5"]
    x = util.shape_corpus(n0, d).numpy()
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    pqt = util.shape_pq_tables(d, m, K, n0)
    vec, pq = gpu.VectorIndex(ids, x), gpu.PQIndex(pqt["codebook"], ids, pqt["codes"])
    rng = np.random.default_rng(23)
    qs = (x[rng.choice(n0, AS_MAX_Q)] * np.float32(0.5) + x[rng.choice(n0, AS_MAX_Q)] * np.float32(0.5)).astype(np.float32)
    qs[60000] = qs[77]
    tg = np.array([77, 1999, n0 + 1], np.int32)
    assert am.same(vec.assign(qs, tg), am.exact_assign(ids, x, qs, tg))
    assert am.same(pq.assign(qs, tg), am.pq_assign(oracle, pqt["codebook"], ids, pqt["codes"], qs, tg))
    with pytest.raises(gpu.FreddyGpuError, match="Q=65537 exceeds"):
        vec.assign(np.zeros((AS_MAX_Q + 1, d), np.float32), tg)
    vec.close(); pq.close()


def test_sentinel_and_empty_calls(tabs, oracle):
    from freddy_amd import gpu
    t = tabs
    tg, qs = t["targets"][:65], t["cent"][:5]
    d = am.adc_dists(oracle, t["cb"], t["codes"][tg[0] - 1][None, :], qs)[0]
    for sentinel in (float(np.sort(d)[2]), 0.0, -1.0, 16777216.0):        # strict "<": the third smallest distance itself is out
        assert am.same(t["pq"].assign(qs, tg, sentinel=sentinel), am.pq_assign(oracle, t["cb"], t["ids"], t["codes"], qs, tg, sentinel=sentinel))
    q, s = t["pq"].assign(qs, tg, sentinel=0.0)
    assert (q == -1).all() and np.isneginf(s).all()
    for ix in (t["vec"], t["pq"]):
        q, s = ix.assign(qs, np.zeros(0, np.int32))
        assert q.size == 0 and s.size == 0
        q, s = ix.assign(np.zeros((0, qs.shape[1]), np.float32), tg)      # no query: nothing is written
        assert q.size == 65
    with pytest.raises(gpu.FreddyGpuError, match="error -4"):              # FREDDY_E_KIND
        gpu._assign(t["pq"], t["pq"].lib.freddy_gpu_exact_assign, qs, tg, ())
    with pytest.raises(gpu.FreddyGpuError, match="error -4"):
        gpu._assign(t["vec"], t["vec"].lib.freddy_gpu_pq_assign, qs, tg, (gpu.C.c_float(1000.0),))


# ---- against the path it replaces, on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [90, 4096])
def test_assign_equals_the_lists_it_replaces(tabs, oracle, n):
    """freddy_gpu_exact_join / freddy_gpu_pq_search at k = n, their rows ordered by (similarity DESC, query, token) and the first row
    of every token kept: what generic_cluster's loop did with them."""
    t = tabs
    rng = np.random.default_rng(n)
    tokens = np.sort(rng.choice(t["ids"], n, replace=False)).astype(np.int32)
    qs = t["cent"][:5]
    ids, sims = t["vec"].join(qs, n, tokens)
    rows = [(sims[qi, r], qi + 1, int(np.searchsorted(tokens, ids[qi, r])) + 1) for qi in range(5) for r in range(n) if ids[qi, r] >= 0]
    assert len(rows) == 5 * n
    assert am.same(t["vec"].assign(qs, tokens), am.first_per_token(rows, n))
    ids, dist = t["pq"].search(qs, n, sentinel=1000.0, subset_ids=tokens)
    sim = am.similarity_of(oracle, np.where(ids >= 0, dist, np.float32(0)))
    rows = [(sim[qi, r], qi + 1, int(np.searchsorted(tokens, ids[qi, r])) + 1) for qi in range(5) for r in range(n) if ids[qi, r] >= 0]
    assert len(rows) == 5 * n
    assert am.same(t["pq"].assign(qs, tokens, sentinel=1000.0), am.first_per_token(rows, n))


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "neg_nan", "pos_inf", "both_inf"])
def test_poisoned_queries(tabs, oracle, kind):
    """One query of 17 is poisoned (tests/util.poison_query, as test_gpu_nonfinite.py): both calls equal the model, and no target's
    answer among the healthy queries moves -- except where PostgreSQL's order lets the NaN similarity win (exact), while a NaN or
    infinite distance is never below the sentinel (pq)."""
    t = tabs
    m = SHAPES[t["shape"]][1]
    tg = t["targets"][:130]
    qs = t["cent"][:17].copy()
    healthy = np.delete(np.arange(17), 9)
    qs[9] = util.poison_query(qs[9], kind, m, np.random.default_rng(3))
    got = t["vec"].assign(qs, tg)
    assert am.same(got, am.exact_assign(t["ids"], t["x"], qs, tg))
    base = t["vec"].assign(qs[healthy], tg)
    kept = got[0] != 9
    assert np.array_equal(got[0][kept], np.where(base[0][kept] >= 0, healthy[np.maximum(base[0][kept], 0)], -1))
    assert np.array_equal(got[1][kept].view(np.uint32), base[1][kept].view(np.uint32))
    if kind in ("nan", "neg_nan"):      # its similarity is a NaN for every row, and a NaN is above every number
        have = am.rows_of(t["ids"], tg) >= 0
        assert (got[0][have] == 9).all() and np.isnan(got[1][have]).all()
    got = t["pq"].assign(qs, tg)
    assert am.same(got, am.pq_assign(oracle, t["cb"], t["ids"], t["codes"], qs, tg))
    base = t["pq"].assign(qs[healthy], tg)
    assert not (got[0] == 9).any()       # its distances are NaN or +Inf: never below the sentinel
    kept = got[0] != 9
    assert np.array_equal(got[0][kept], np.where(base[0][kept] >= 0, healthy[np.maximum(base[0][kept], 0)], -1))
    assert np.array_equal(got[1][kept].view(np.uint32), base[1][kept].view(np.uint32))


def test_nan_row_and_nan_codeword(tabs, oracle):
    from freddy_amd import gpu
    t = tabs
    n0 = 2000
    x, cb = t["x"][:n0].copy(), t["cb"].copy()
    x[7, 3] = np.nan; x[64, x.shape[1] - 1] = np.inf; x[65, 0] = -np.inf
    code = int(t["codes"][11, 0])
    cb[0, code, 1] = np.nan                                           # every row with this code at position 0
    cb[cb.shape[0] - 1, int(t["codes"][12, -1]), 0] = np.inf
    vec = gpu.VectorIndex(t["ids"][:n0], x)
    pq = gpu.PQIndex(cb, t["ids"][:n0], t["codes"][:n0])
    tg = np.concatenate([np.arange(1, 131), np.flatnonzero(t["codes"][:n0, 0] == code)[:20] + 1]).astype(np.int32)
    qs = t["cent"][:17]
    got = vec.assign(qs, tg)
    assert am.same(got, am.exact_assign(t["ids"][:n0], x, qs, tg))
    assert np.isnan(got[1][7]) and got[0][7] == 0                    # the row's similarities are all NaN: the first query
    got = pq.assign(qs, tg)
    assert am.same(got, am.pq_assign(oracle, cb, t["ids"][:n0], t["codes"][:n0], qs, tg))
    assert got[0][11] == -1 and np.isneginf(got[1][11])              # every distance of that row is NaN: no candidate
    vec.close(); pq.close()


# ---- after append_rows -----------------------------------------------------------------------------------------------------
def test_appended_rows_are_assignable(tabs):
    from freddy_amd import gpu
    t = tabs
    cut = N - 700
    tg = np.concatenate([t["targets"][:200], np.arange(cut - 5, N + 3)]).astype(np.int32)
    qs = t["cent"][:17]
    vec = gpu.VectorIndex(t["ids"][:cut], t["x"][:cut])
    before = vec.assign(qs, tg)
    new = tg > cut                                  # the appended ids (and two beyond the table)
    assert (before[0][new] == -1).all() and (before[0][~new] >= 0).any()
    vec.append_rows(t["ids"][cut:], vectors=t["x"][cut:])
    assert am.same(vec.assign(qs, tg), t["vec"].assign(qs, tg))
    vec.close()
    pq = gpu.PQIndex(t["cb"], t["ids"][:cut], t["codes"][:cut])
    pq.append_rows(t["ids"][cut:], codes=t["codes"][cut:])
    got = pq.assign(qs, tg)
    assert am.same(got, t["pq"].assign(qs, tg)) and (got[0][new & (tg <= N)] >= 0).all() and (new & (tg <= N)).sum() >= 700
    pq.close()


# ---- through the host mirror: cluster_exact / cluster_pq ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db(oracle):
    from freddy_amd import udf
    x = util.corpus(N).numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    pq = util.pq_tables(N=N, K=256)
    s = udf.Session()
    s.load_vecs_norm(ids, x)
    s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
    yield s, dict(x=x, ids=ids, pq=pq, pt=oracle.pq_table(pq["codebook"], pq["ids"], pq["codes"]))
    s.close()


def _model_rows(which, t, oracle, tokens):
    def rows(cent):
        if which == "exact":
            q, s = am.exact_assign(t["ids"], t["x"], cent, tokens)
        else:
            q, s = am.pq_assign(oracle, t["pq"]["codebook"], t["pq"]["ids"], t["pq"]["codes"], cent, tokens, sentinel=1000.0)
        return [(s[i], int(q[i]) + 1, i + 1) for i in range(len(tokens)) if q[i] >= 0]
    return rows


@pytest.mark.parametrize("which", ["exact", "pq"])
def test_cluster_over_5000_tokens(db, oracle, which):
    """n = 5000 tokens, k = 7, supplied draws: the ten rounds reproduce generic_cluster's restatement fed by the model.  (With lists of
    all tokens per centroid this call was refused: k = n > 4096, FREDDY_E_LIMIT.)  The profile names the assign kernel and no
    selection pass of the big-k path."""
    from test_gpu_udf import _cluster_reference
    s, t = db
    rng = np.random.default_rng(41)
    n, k = 5000, 7
    tokens = np.sort(rng.choice(t["ids"], n, replace=False)).astype(np.int32)
    draws = rng.random(k + 9 * k * 10)
    exp = _cluster_reference(_model_rows(which, t, oracle, tokens), t["x"][tokens - 1], n, k, draws)
    s.exact_assign(t["x"][:1], tokens[:1]) if which == "exact" else None      # (pins the vectors: the handle exists before it is profiled)
    idx = s.gpu_index("vecs" if which == "exact" else "pq")
    idx.profile_enable(True)
    got = getattr(s, "cluster_" + which)(tokens, k, draws)
    names = set(idx.profile_read())
    idx.profile_enable(False)
    assert np.array_equal(got, exp), f"cluster_{which}: {np.flatnonzero(got != exp)[:10]}"
    assert set(np.unique(got)) <= set(range(1, k + 1))
    assert f"assign_{which}_kernel" in names, names
    assert not [x for x in names if "bigk" in x or "select" in x or "merge" in x or "scan" in x], names


@pytest.mark.parametrize("which", ["exact", "pq"])
def test_cluster_over_90_tokens_equals_the_list_based_rows(db, oracle, which):
    """n = 90: the restatement fed by the rows of the lists (as test_gpu_udf.test_cluster_functions) and fed by the model give the
    same clusters, and the device gives them too."""
    from test_gpu_udf import _cluster_reference, _sim_of
    s, t = db
    rng = np.random.default_rng(43)
    n, k = 90, 5
    tokens = np.sort(rng.choice(t["ids"], n, replace=False)).astype(np.int32)
    draws = rng.random(k + 9 * k * 10)

    def list_rows(cent):
        if which == "exact":
            out = []
            for qi, c in enumerate(cent):
                e = oracle.exact_knn(t["x"], t["ids"], c, n, tokens)
                out += [(np.float32(e["dist"][r]), qi + 1, int(np.searchsorted(tokens, e["id"][r])) + 1) for r in range(len(e))]
            return out
        e = oracle.pq_search_in_batch(t["pt"], cent, n, tokens)
        return [(_sim_of(oracle, e["dist"][qi, r]), qi + 1, int(np.searchsorted(tokens, e["id"][qi, r])) + 1)
                for qi in range(len(cent)) for r in range(n) if e["id"][qi, r] >= 0]

    vecs = t["x"][tokens - 1]
    exp_lists = _cluster_reference(list_rows, vecs, n, k, draws)
    exp_model = _cluster_reference(_model_rows(which, t, oracle, tokens), vecs, n, k, draws)
    got = getattr(s, "cluster_" + which)(tokens, k, draws)
    assert np.array_equal(exp_lists, exp_model)
    assert np.array_equal(got, exp_lists), f"cluster_{which}: {np.flatnonzero(got != exp_lists)[:10]}"


def test_session_assign_calls(db, oracle):
    s, t = db
    rng = np.random.default_rng(47)
    cent = np.stack([t["x"][rng.choice(N, 10)].mean(axis=0) for _ in range(7)]).astype(np.float32)
    tg = np.array([5, 5, 19999, N + 1, 17], np.int32)
    assert am.same(s.exact_assign(cent, tg), am.exact_assign(t["ids"], t["x"], cent, tg))
    assert am.same(s.pq_assign(cent, tg), am.pq_assign(oracle, t["pq"]["codebook"], t["pq"]["ids"], t["pq"]["codes"], cent, tg, sentinel=1000.0))


# ---- many targets: four targets per thread, a second pass; LUTs that fill the LDS ------------------------------------------------
def _in_chunks_of_1000(ix, qs, tg):
    """The same call 1000 targets at a time: one target per thread in assign_pq_kernel, the path test_assign_equals_the_model ties to
    the model at n = 1000."""
    parts = [ix.assign(qs, tg[i:i + 1000]) for i in range(0, tg.size, 1000)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _all_ids_shuffled(ids, seed):
    base = np.random.default_rng(seed).permutation(ids).astype(np.int32)
    base[[7, 999, 1000, 14309, 19999]] = [N + 1, -2, 2**31 - 1, N + 2, 0]        # ids without a row, at the ends of chunks too
    return base


def test_pq_assign_over_600000_targets(tabs, oracle):
    """n = 600 037 (the 20 000 ids 30 times and 37 more; not a multiple of the 1024 targets of a workgroup): from 256 CUs x 2 x 4 x 256
    = 524 288 targets on freddy_gpu_pq_assign takes assign_pq_kernel<., 4>, four targets per thread.  The result must be that of
    the same targets 1000 at a time, which are the same 20 calls again and again, so they are made once and repeated."""
    t = tabs
    qs = t["cent"][:5]                                               # (the fifth repeats the first: it must win nowhere)
    base = _all_ids_shuffled(t["ids"], 29)
    ref = _in_chunks_of_1000(t["pq"], qs, base)
    assert am.same((ref[0][:1000], ref[1][:1000]), am.pq_assign(oracle, t["cb"], t["ids"], t["codes"], qs, base[:1000]))
    n = 30 * N + 37
    assert n >= 256 * 2 * 4 * 256 and n % 1024
    got = t["pq"].assign(qs, np.resize(base, n))
    assert am.same(got, (np.resize(ref[0], n), np.resize(ref[1], n))), np.flatnonzero(got[0] != np.resize(ref[0], n))[:8]
    assert (ref[0][[7, 999, 1000, 19999]] == -1).all() and not (got[0] == 4).any()


def test_assign_over_more_than_one_pass_of_targets(oracle):
    """n = 2^22 + 1000 targets, Q = 1, the 25-d shape: both entry points walk the targets in passes of 2^22, the second one of 1000
    here (for the PQ kernel the first with four targets per thread, the second with one).  Compared with the same targets 1000 at
    a time, as above."""
    from freddy_amd import gpu
    x, ids, cb, codes = _tables("25d_m5")
    vec, pq = gpu.VectorIndex(ids, x), gpu.PQIndex(cb, ids, codes)
    qs = x[np.random.default_rng(31).choice(N, 10)].mean(axis=0, dtype=np.float32)[None, :]
    base = _all_ids_shuffled(ids, 37)
    n = 2**22 + 1000
    tg = np.resize(base, n)
    for ix, model in ((vec, lambda g: am.exact_assign(ids, x, qs, g)), (pq, lambda g: am.pq_assign(oracle, cb, ids, codes, qs, g))):
        ref = _in_chunks_of_1000(ix, qs, base)
        assert am.same((ref[0][:1000], ref[1][:1000]), model(base[:1000]))
        got = ix.assign(qs, tg)
        exp = (np.resize(ref[0], n), np.resize(ref[1], n))
        assert am.same(got, exp), np.flatnonzero(got[0] != exp[0])[:8]
        # the five ids without a row: 209 whole repeats and four of them again in the rest, the one at 14309 in the second pass
        assert (got[0] == -1).sum() == 5 * (n // N) + 4 and (got[0][2**22:] == -1).sum() == 1 and 2**22 % N <= 14309 < 2**22 % N + 1000
    vec.close(); pq.close()


@pytest.mark.parametrize("d,m,K", [(300, 12, 1024), (300, 12, 2048), (25, 5, 4096)])
def test_pq_assign_with_one_lut_per_stage(oracle, d, m, K):
    """LUTs of 48, 96 and 80 KiB: only one fits a stage in LDS (LT = 1; Q = 5 is five stages), and the larger two ask for more than
    the default 64 KiB of dynamic LDS (lds_limits_pq), with the codes in registers (m = 12) and re-read per query (m = 5).  The
    codebook is rows' own subvectors and the codes are random: the assignment only needs a table, not a good one."""
    from freddy_amd import gpu
    n0, rng = 2000, np.random.default_rng(K + m)
    x = (util.corpus(n0) if d == 300 else util.shape_corpus(n0, d)).numpy()
    ids = np.arange(1, n0 + 1, dtype=np.int32)
    S = d // m
    cb = np.stack([x[rng.choice(n0, K), p * S:(p + 1) * S] for p in range(m)]).astype(np.float32)     # [m][K][S]
    codes = rng.integers(0, K, (n0, m)).astype(np.int32)
    codes[0] = K - 1; codes[1] = 0                                                                       # the LUT's ends
    pq = gpu.PQIndex(cb, ids, codes)
    qs = np.stack([x[rng.choice(n0, 10)].mean(axis=0) for _ in range(5)]).astype(np.float32)
    qs[3] = qs[1]
    tg = np.concatenate([[1, 2, n0 + 5, 2], rng.choice(ids, 296)]).astype(np.int32)
    got = pq.assign(qs, tg)
    assert am.same(got, am.pq_assign(oracle, cb, ids, codes, qs, tg))
    assert got[0][2] == -1 and (np.delete(got[0], 2) >= 0).all() and not (got[0] == 3).any()
    pq.close()
