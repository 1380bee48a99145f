"""The draws of the randomised fixed-seed soaks: plain numpy and the CPU oracle, no device.

One function per family, draw_<family>(seed, oracle=None) -> dict: the shapes and options, the arrays, and the expected answers
computed through the oracle and the numpy models the tests already have (analogy_model, pair_model, pv_model,
approx_analogy_model, assign_model, update_model).  Everything follows from np.random.default_rng(BASE[family] + seed); every dict
carries a one-line "label" with all drawn parameters, which every assertion message of the GPU tests includes, so a failing seed
can be reproduced from the log alone.  The pools are small sets placed on the thresholds in the code; a threshold that lives in
a header is read from there (constant()).

  tests/test_soak_inputs_cpu.py   proves on the CPU that the seed lists below reach every regime the soaks are about;
  tests/test_gpu_soak*.py         run the draws against the handles;
  tools/soak_*.py                 loop over the same draws for any seed count.

SEEDS[family] is the list the GPU tests parametrise over and the CPU test proves; a seed is never taken out of it to make a run
pass."""
import os
import re

import numpy as np

import analogy_model as am
import approx_analogy_model as aam
import assign_model as asm
import pair_model as pam
import pv_model as pm
import update_model as um

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "postgres-word2vec_amd", "csrc")

# shapes, bigk and join keep the bases of the tools they come from.  The others are arbitrary; exact's was taken from a scan of
# 21000 .. 22999 for the base whose first seeds walk all 42 ordered pairs of call kinds soonest (15 seeds; 28 at 21000) -- a
# property of the draws alone, which tests/test_soak_inputs_cpu.py asserts.
BASE = {"shapes": 1000, "bigk": 5000, "join": 9000, "exact": 21603, "rerank": 33000, "mutation": 47000}
SEEDS = {"shapes": list(range(11)), "bigk": list(range(8)), "join": list(range(8)), "exact": list(range(32)),
         "rerank": list(range(16)), "mutation": list(range(8))}
MUTATION_KINDS = ("pq", "ivf", "ivpq", "vec")

# the index shapes of tools/soak_shapes.py: (d, m, K)
SHAPES = [(25, 5, 256), (300, 6, 256), (300, 10, 64), (300, 15, 128), (300, 30, 32), (300, 4, 512), (300, 20, 16), (300, 12, 256),
          (300, 12, 1024), (50, 10, 256), (64, 8, 128)]
N_CAP, Q_CAP = 40000, 130

_oracle = []


def the_oracle(oracle=None):
    """the session's oracle where the caller has one, else one per process"""
    if oracle is not None:
        return oracle
    if not _oracle:
        from oracle.oracle import Oracle
        _oracle.append(Oracle())
    return _oracle[0]


def constant(source, name):
    """static constexpr <integer type> NAME = <expr of integers and earlier constants>; read from a file of csrc/"""
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(r"static constexpr (?:int|int64_t|size_t) " + name + r" = ([^;]+);", text)
    assert m, (source, name)
    expr = re.sub(r"[A-Z][A-Z0-9_]+", lambda dep: str(constant(source, dep.group(0))), m.group(1))
    assert re.fullmatch(r"[0-9 */+()-]+", expr), expr
    return int(eval(expr))   # noqa: S307 (digits and operators only, checked above)


def exj_min_targets():
    return constant("exact.hip", "EXJ_MIN_TARGETS")


def exf_sample():
    return constant("exact2.h", "EXF_SAMPLE")


def exf_pass():
    return constant("exact2.h", "EXF_QT")


def analogy_pass():
    return constant("analogy.h", "AN_PASS")


def analogy_max_k():
    return constant("analogy.h", "AN_MAXK")


def pv_max_cand():
    return constant("pv.h", "PV_MAX_CAND")


EXF_AUTO_ROWS = constant("exact_host.h", "EXF_AUTO_ROWS")   # exf_wanted: "exact_filter == 1 || n_rows >= auto_rows" of the three entry points


def filter_eligible(d):
    """internal.h, exf_ok: d % 4 == 0 and d <= 512 (and every element finite, which the draws' tables are)"""
    return d % 4 == 0 and d <= 512


# =======================================================================================
# shapes: tools/soak_shapes.py -- the IVFADC search on index shapes other than m = 12 / S = 25
# =======================================================================================
SHAPES_CONFIGS = ((-1, 1), (1, 1), (1, 0), (0, 1))   # (fused, running_bound) of every call


def _ivf_build(x, C, m, K, seed):
    from freddy_amd import index_build as ib
    return ib.build_ivf_index(x, C=C, m=m, K=K, train_size=min(x.shape[0], 4000), iters=3, seed=seed)


def _corpus_torch(N, d, seed, n_clusters, dup_frac):
    import torch
    from freddy_amd import index_build as ib
    torch.manual_seed(seed)
    return ib.make_corpus(N, d=d, seed=seed, n_clusters=n_clusters, latent=min(10, d), dup_frac=dup_frac, device="cpu")


def draw_shapes(seed, oracle=None):
    """The shape comes from a fixed shuffle of SHAPES walked by the seed (len(SHAPES) consecutive seeds draw every entry); the
    rest as tools/soak_shapes.py drew it, N capped at N_CAP and Q at Q_CAP."""
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["shapes"] + seed)
    order = np.random.default_rng(BASE["shapes"]).permutation(len(SHAPES))
    d, m, K = SHAPES[int(order[seed % len(SHAPES)])]
    N = int(rng.choice([900, 5000, 30000, N_CAP]))
    C = int(rng.choice([1, 3, 16, 40, 200]))
    C = min(C, max(1, N // 20))
    x = _corpus_torch(N, d, seed, 60, 0.02)
    t = _ivf_build(x, C, m, K, seed)
    pin = (t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    ot = o.ivf_table(*pin)
    Q = int(rng.choice([1, 7, 40, 65, Q_CAP]))
    qs = x.numpy()[rng.integers(0, N, size=Q)].astype(np.float32) * np.float32(rng.choice([1.0, 1.0, 1.02]))
    label = f"shapes seed={seed} d={d} m={m} K={K} N={N} C={C} Q={Q}"
    calls = []
    for (W, k, rule, sent) in [(int(rng.choice([1, 2, 5])), int(rng.choice([1, 5, 20, 32])), 0, 1000.0), (1, 5, 2, 100.0), (3, 10, 1, 100.0)]:
        W = min(W, C)
        exp = o.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule, n_threads=8)
        calls.append({"k": k, "W": W, "rule": rule, "sentinel": sent, "exp": exp})
    label += " calls=" + ",".join(f"(W={c['W']} k={c['k']} rule={c['rule']})" for c in calls)
    return {"label": label, "shape": (d, m, K), "N": N, "C": C, "Q": Q, "pin": pin, "qs": qs, "calls": calls}


# =======================================================================================
# bigk: tools/soak_bigk.py -- lists of 513 .. 4096 entries, the join's post verification of 1025 .. 8192 candidates
# =======================================================================================
def draw_bigk(seed, oracle=None):
    from freddy_amd import index_build as ib
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["bigk"] + seed)
    N = int(rng.choice([3000, 12000, N_CAP]))
    d, m, K = [(300, 12, 256), (300, 12, 1024), (50, 10, 64), (300, 6, 256)][int(rng.integers(0, 4))]
    C = int(rng.choice([1, 8, 40]))
    dup = float(rng.choice([0.02, 0.3]))
    x = _corpus_torch(N, d, seed, 40, dup)
    label = f"bigk seed={seed} d={d} m={m} K={K} N={N} C={C} dup={dup}"
    # ---- IVFADC
    t = dict(_ivf_build(x, C, m, K, seed))
    codes = t["codes"].copy()
    lo = t["list_off"]
    for c in range(len(lo) - 1):   # runs of equal code rows: equal distances around the k-th place
        n = min(int(rng.integers(0, 700)), int(lo[c + 1] - lo[c]))
        if n:
            codes[lo[c]:lo[c] + n] = codes[lo[c]]
    t["codes"] = codes
    ivf_pin = (t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    ot = o.ivf_table(*ivf_pin)
    Q = int(rng.choice([1, 3, 9]))
    qs = x.numpy()[rng.integers(0, N, size=Q)].astype(np.float32)
    label += f" Q={Q}"
    ivf_calls = []
    for _ in range(3):
        k = int(rng.choice([513, 700, 1024, 1025, 1500, 2048, 3000, 4096]))
        W = min(int(rng.choice([1, 2, 5])), C)
        rule, sent = [(0, 1000.0), (1, 1000.0), (0, float(rng.choice([0.5, 2.0, 8.0]))), (2, 100.0)][int(rng.integers(0, 4))]
        if rule == 2:
            W = 1
        exp = o.ivfadc_search_many(ot, qs, k, W, sentinel=sent, found_rule=rule, n_threads=8)
        ivf_calls.append({"k": k, "W": W, "rule": rule, "sentinel": sent, "exp": exp})
    label += " ivf=" + ",".join(f"(k={c['k']} W={c['W']} rule={c['rule']} sent={c['sentinel']})" for c in ivf_calls)
    # ---- PQ
    tp = ib.build_pq_index(x, m=m, K=K, train_size=min(N, 4000), iters=3, seed=seed)
    pcodes = tp["codes"].copy()
    a = int(rng.integers(0, N // 2))
    pcodes[a:a + int(rng.integers(1, 1500))] = pcodes[a]
    pq_pin = (tp["codebook"], tp["ids"], pcodes)
    op = o.pq_table(*pq_pin)
    pk = int(rng.choice([513, 900, 2048, 4096]))
    pq_exp = np.stack([o.pq_search(op, q, pk) for q in qs])
    targets = rng.choice(np.arange(1, N + 1), size=min(N, int(rng.choice([pk - 7, 2 * pk, N // 2]))), replace=False).astype(np.int32)
    pq_in_exp = o.pq_search_in_batch(op, qs, pk, targets, use_target_lists=True)
    label += f" pq_k={pk} pq_targets={targets.size}"
    out = {"label": label, "shape": (d, m, K), "N": N, "C": C, "Q": Q, "qs": qs, "ivf_pin": ivf_pin, "ivf_calls": ivf_calls,
           "pq_pin": pq_pin, "pq_k": pk, "pq_exp": pq_exp, "pq_targets": targets, "pq_in_exp": pq_in_exp, "join": None}
    # ---- kNN-join, post verification of more than 1024 candidates
    if d == 300 and seed % 2 == 0:
        tj = ib.build_ivpq_index(x, m=30, K=32, k_coarse=8, train_size=min(N, 4000), iters=3, seed=seed)
        pin = (tj["codebook"], tj["coarse"], tj["ids"], tj["coarse_id"], tj["codes"], tj["vectors"], tj["stats"])
        oj = o.ivpq_table(*pin)
        tg = rng.choice(np.arange(1, N + 1), size=int(N * float(rng.choice([0.2, 0.8]))), replace=False).astype(np.int32)
        jq = x.numpy()[rng.integers(0, N, size=12)].astype(np.float32)
        calls = []
        for _ in range(2):
            kj = int(rng.choice([20, 60, 100, 400]))
            pvf = int(rng.choice([p for p in (20, 50, 100, 400) if 1024 < kj * p <= 8192] or [8192 // kj]))
            alpha = int(rng.choice([3, 30, 200]))
            use_tl = bool(rng.integers(0, 2))
            exp, eit = o.ivpq_search_in(oj, jq, kj, tg, alpha, pvf, 2, use_target_lists=use_tl, confidence=0.8)
            calls.append({"k": kj, "pvf": pvf, "alpha": alpha, "tl": use_tl, "exp": exp, "iterations": eit})
        out["join"] = {"pin": pin, "targets": tg, "qs": jq, "calls": calls}
        out["label"] += f" join_targets={tg.size} join=" + ",".join(f"(k={c['k']} pvf={c['pvf']} alpha={c['alpha']} tl={c['tl']})" for c in calls)
    return out


# =======================================================================================
# join: the kNN-join part of tools/soak_round3.py -- the traversal on the device and on the host heap
# =======================================================================================
def draw_join(seed, oracle=None):
    from freddy_amd import index_build as ib
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["join"] + seed)
    Nj = int(rng.choice([3000, 20000]))
    kc = int(rng.choice([4, 8, 32]))
    xj = ib.make_corpus(Nj, seed=200 + seed, n_clusters=40, dup_frac=0.02, device="cpu")
    tj = dict(ib.build_ivpq_index(xj, m=30, K=32, k_coarse=kc, train_size=min(Nj, 3000), iters=3, seed=seed))
    dup_centroids = seed % 4 == 1
    if dup_centroids:   # duplicate multi-index centroids: equal keys among the nearest cells
        co = tj["coarse"].copy()
        co[0, 1] = co[0, 0]
        co[1, kc - 1] = co[1, 0]
        tj["coarse"] = co
    pin = (tj["codebook"], tj["coarse"], tj["ids"], tj["coarse_id"], tj["codes"], tj["vectors"], tj["stats"])
    otj = o.ivpq_table(*pin)
    Qj = int(rng.choice([1, 40, Q_CAP]))
    qj = xj.numpy()[rng.integers(0, Nj, size=Qj)].astype(np.float32)
    T = int(rng.choice([5, 200, Nj // 4]))
    targets = rng.choice(np.arange(1, Nj + 1), size=T, replace=False).astype(np.int32)
    calls = []
    for _ in range(3):
        k = int(rng.choice([1, 5, 12]))
        alpha = int(rng.choice([1, 3, 50, 1000]))
        pvf = int(rng.choice([1, 4, 20]))
        method = int(rng.choice([0, 1, 2]))
        conf = float(rng.choice([0.05, 0.5, 0.8, 0.99]))
        tl = bool(rng.integers(0, 2))
        exp, eit = o.ivpq_search_in(otj, qj, k, targets, alpha, pvf, method, use_target_lists=tl, confidence=conf)
        calls.append({"k": k, "alpha": alpha, "pvf": pvf, "method": method, "confidence": conf, "tl": tl, "exp": exp, "iterations": eit})
    label = (f"join seed={seed} N={Nj} kc={kc} dup_centroids={dup_centroids} Q={Qj} T={T} calls="
             + ",".join(f"(k={c['k']} alpha={c['alpha']} pvf={c['pvf']} method={c['method']} conf={c['confidence']} tl={c['tl']})" for c in calls))
    return {"label": label, "N": Nj, "kc": kc, "Q": Qj, "pin": pin, "qs": qj, "targets": targets, "calls": calls}


# =======================================================================================
# exact: one VectorIndex per seed, 6 - 8 calls in a random order on the same handle
# =======================================================================================
EXACT_KINDS = ("search", "search_subset", "join", "assign", "3cosadd", "3cosmul", "pair_direction")
EXACT_D = (16, 25, 64, 100, 300, 301, 304, 512, 516)
EXACT_N = (20, 33, 2080, 8191, 8192, 33000, 40000)
EXACT_Q = (1, 9, 64, 65, 130)
EXACT_K = (1, 5, 32, 33, 200)
ORACLE_BUDGET = 1.0e9       # N * d * Q of the whole-table oracle.exact_knn of a seed (the subset calls take the rest of 2e9)
MODEL_BUDGET = 3.0e8        # elements * steps of one numpy model call (analogy_model, pair_model, assign_model)
ANALOGY_COST = {"3cosadd": 1, "3cosmul": 3, "pair_direction": 4}


def numpy_corpus(rng, N, d, dup_frac=0.02):
    """N x d float32 unit rows clustered in min(10, d) latent dimensions (index_build.make_corpus in numpy), dup_frac of them (at
    least one) exact copies of other rows: equal similarities, the id decides."""
    latent = min(10, d)
    nc = max(2, min(60, N // 4))
    centers = rng.standard_normal((nc, latent))
    lift = rng.standard_normal((latent, d)) / np.sqrt(latent)
    z = centers[rng.integers(0, nc, size=N)] + 0.35 * rng.standard_normal((N, latent))
    v = z @ lift + 0.01 * rng.standard_normal((N, d))
    x = np.ascontiguousarray((v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)).astype(np.float32))
    n_dup = max(1, int(N * dup_frac))
    dst = rng.choice(N, size=n_dup, replace=False)
    x[dst] = x[rng.integers(0, N, size=n_dup)]
    return x


def gapped_ids(rng, N, first=3):
    """ascending int32 ids with gaps of 0 - 2 ids between neighbours: every gap holds ids no row has"""
    return (first + np.cumsum(rng.integers(1, 4, size=N)) - 1).astype(np.int32)


def unknown_ids(rng, ids, n=6):
    """ids no row has: inside gaps, below the first, above the last, negative"""
    near = np.setdiff1d(ids[rng.integers(0, ids.size, size=n)].astype(np.int64) + 1, ids)
    return np.concatenate([near, [int(ids[0]) - 1, int(ids[-1]) + 5, 10 ** 8, -7]]).astype(np.int32)


def id_set(rng, ids, n_known):
    """n_known distinct known ids (all of them where the table has fewer), 2 % of them twice, unknown ids among them; shuffled"""
    rows = rng.choice(ids.size, size=min(n_known, ids.size), replace=False)
    twice = rows[:max(1, rows.size // 50)]
    out = np.concatenate([ids[rows], ids[twice], unknown_ids(rng, ids)])
    return rng.permutation(out).astype(np.int32)


def subset_sizes(N):
    """distinct known rows of a subset: a handful, a few strips, and either side of the join's EXJ_MIN_TARGETS"""
    t = exj_min_targets()
    return [3, 70] + [v for v in (t - 1, t, t + 300) if v <= N] + ([max(1, N // 2), N] if N < t + 300 else [])


def _fits(pool, unit, budget):
    ok = [v for v in pool if v * unit <= budget]
    return ok or [min(pool)]


def exact_sequence(rng):
    """6 - 8 positions in EXACT_KINDS, never the same kind twice in a row: every step is a change of path"""
    n_calls = int(rng.integers(6, 9))
    kinds = [int(rng.integers(0, len(EXACT_KINDS)))]
    while len(kinds) < n_calls:
        nxt = int(rng.integers(0, len(EXACT_KINDS) - 1))
        kinds.append(nxt + (nxt >= kinds[-1]))
    return kinds


def draw_exact(seed, oracle=None):
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["exact"] + seed)
    d = int(rng.choice(EXACT_D))
    N = int(rng.choice(EXACT_N))
    Q_drawn = int(rng.choice(EXACT_Q))
    Q = max(_fits([q for q in EXACT_Q if q <= Q_drawn], N * d, ORACLE_BUDGET))
    k = int(rng.choice(EXACT_K))
    exact_filter = int(rng.choice([-1, 1]))
    refine_all = seed % 3 == 1        # option check_brackets bits 2 and 3 ("exact_refine_all"): every row is refined and checked
    kinds = exact_sequence(rng)
    x = numpy_corpus(rng, N, d)
    ids = gapped_ids(rng, N)
    # one row with `clump` exact copies and a query equal to it: a run of bit-equal similarities at the top of that query's list
    anchor = int(rng.integers(0, N))
    clump = int(rng.choice([1, min(k, N - 1), min(k + 2, N - 1)]))
    copies = rng.choice(np.setdiff1d(np.arange(N), [anchor]), size=clump, replace=False)
    x[copies] = x[anchor]
    qs = x[rng.integers(0, N, size=Q)].copy()
    qs[0] = x[anchor]
    if Q > 1:
        qs[1] = -qs[1]                                     # negative similarities
    if Q > 2:
        qs[2::5] += (0.05 * rng.standard_normal(qs[2::5].shape)).astype(np.float32)   # queries that are no rows, not normalised
    x_t = np.ascontiguousarray(x.T)
    ka = min(k, analogy_max_k())
    label = (f"exact seed={seed} d={d} N={N} Q={Q} (drawn {Q_drawn}) k={k} exact_filter={exact_filter} refine_all={int(refine_all)} "
             f"anchor={anchor} clump={clump}")
    whole = None
    calls = []
    for ci, kind in enumerate(EXACT_KINDS[i] for i in kinds):
        call = {"kind": kind}
        if kind == "search":
            if whole is None:
                whole = [o.exact_knn(x, ids, q, k) for q in qs]
            call.update(exp=whole, what="")
        elif kind in ("search_subset", "join"):
            sub = id_set(rng, ids, int(rng.choice(subset_sizes(N))))
            call.update(ids=sub, exp=[o.exact_knn(x, ids, q, k, sub) for q in qs], what=f"n={sub.size}")
        elif kind == "assign":
            n = int(rng.choice(subset_sizes(N)))
            sub = id_set(rng, ids, max(1, min(n, int(MODEL_BUDGET / (Q * d)))))
            call.update(ids=sub, exp=asm.exact_assign(ids, x, qs, sub), what=f"n={sub.size}")
        else:
            ap = analogy_pass()
            Qa = int(rng.choice(_fits([3, ap - 1, ap, ap + 1, 2 * ap + 6], N * d * ANALOGY_COST[kind], MODEL_BUDGET)))
            triples = ids[rng.integers(0, N, size=(Qa, 3))].copy()
            triples[0] = (ids[anchor], ids[copies[0]], ids[int(rng.integers(0, N))])      # two inputs hold one vector
            if Qa > 2:
                triples[1, int(rng.integers(0, 3))] = unknown_ids(rng, ids)[0]               # an unknown input: an empty list
                triples[2, 2] = triples[2, 0]                                                # w1 == w3
            sub = id_set(rng, ids, int(rng.choice(subset_sizes(N)))) if rng.integers(0, 2) else None
            if kind == "pair_direction":
                exp = pam.model(x, ids, triples, ka, subset_ids=sub, x_t=x_t)
            else:
                exp = am.model(x, ids, triples, ka, kind, subset_ids=sub, x_t=x_t)
            call.update(triples=triples, ids=sub, k=ka, exp=exp, what=f"Q={Qa} subset={'-' if sub is None else sub.size}")
        calls.append(call)
        label += f" {ci}:{kind}({call['what']})"
    return {"label": label, "d": d, "N": N, "Q": Q, "Q_drawn": Q_drawn, "k": k, "exact_filter": exact_filter, "refine_all": refine_all,
            "x": x, "ids": ids, "qs": qs, "calls": calls, "kinds": [EXACT_KINDS[i] for i in kinds]}


def exact_ties(draw, oracle=None):
    """those of the draw's first three queries whose k-th and (k + 1)-th similarities over the whole table are bit-equal"""
    o = the_oracle(oracle)
    k = draw["k"]
    if draw["N"] <= k:
        return []
    out = []
    for qi, q in enumerate(draw["qs"][:3]):           # (the planted query is the first)
        bits = o.exact_knn(draw["x"], draw["ids"], q, k + 1)["dist"].view(np.uint32)
        if bits.size == k + 1 and bits[k - 1] == bits[k]:
            out.append(qi)
    return out


# =======================================================================================
# rerank: an IVFIndex or a PQIndex plus the VectorIndex of (most of) the same rows
# =======================================================================================
PV_POOL = ((5, 1), (5, 6), (5, 7), (5, 20), (32, 16), (33, 16), (64, 64))   # (k, pvf): 2 k pvf either side of 64, k pvf of one wave, four waves, 512
NCAND_POOL = (4, 23, 64, 65, 513, 4096)
RERANK_N = (900, 5000, 30000)


def draw_rerank(seed, oracle=None):
    """Even seeds pin an IVFADC table, odd ones a flat PQ table.  The (k, pvf) of the main search_pv call and the n_cand of the
    analogies walk fixed shuffles of their pools by the seed, so that len(pool) consecutive seeds of a kind draw every value; the
    rest is drawn.  3 % of the ids have no vector row; from three triples on, one names such an id (it is not searched) and one
    has v3 - v1 + v2 = 0 exactly (a planted row)."""
    from freddy_amd import index_build as ib
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["rerank"] + seed)
    kind = ("ivf", "pq")[seed % 2]
    d, m, K = SHAPES[int(rng.integers(0, len(SHAPES)))]
    N = int(rng.choice(RERANK_N))
    k, pvf = PV_POOL[int(np.random.default_rng(BASE["rerank"]).permutation(len(PV_POOL))[(seed // 2) % len(PV_POOL)])]
    n_cand = NCAND_POOL[int(np.random.default_rng(BASE["rerank"] + 1).permutation(len(NCAND_POOL))[(seed // 2) % len(NCAND_POOL)])]
    Q = int(rng.choice([1, 9, 65]))
    Qt = int(rng.choice([1, 9, 40]))
    x = _corpus_torch(N, d, BASE["rerank"] + seed, 60, 0.02).numpy().copy()
    ids = np.arange(1, N + 1, dtype=np.int32)                       # (make_corpus: ids 1 .. N in row order)
    a, c, j = (int(v) for v in rng.choice(N, size=3, replace=False))
    x[j] = x[a] - x[c]                                              # the triple (a, j, c): (v_c - v_a) + v_j = 0 in every element
    import torch
    xt = torch.from_numpy(x)
    keep = rng.random(N) >= 0.03
    keep[[a, c, j]] = True
    vec_ids, vec_x = ids[keep], np.ascontiguousarray(x[keep])
    missing = ids[~keep]
    label = f"rerank seed={seed} kind={kind} d={d} m={m} K={K} N={N} Q={Q} triples={Qt} k={k} pvf={pvf} n_cand={n_cand} no_vector={missing.size}"
    qs = x[rng.integers(0, N, size=Q)].copy()
    if Q > 2:
        qs[2] = -qs[2]
    triples = rng.choice(vec_ids, size=(Qt, 3)).astype(np.int32)
    if Qt >= 3:
        triples[1, int(rng.integers(0, 3))] = missing[0]
        triples[2] = (ids[a], ids[j], ids[c])
    ka = min(int(rng.choice([1, 5])), n_cand)
    out = {"kind": kind, "shape": (d, m, K), "N": N, "Q": Q, "k": k, "pvf": pvf, "n_cand": n_cand, "ka": ka, "qs": qs, "triples": triples,
           "vec_pin": (vec_ids, vec_x), "missing": missing}
    if kind == "ivf":
        C = min(int(rng.choice([1, 16, 40])), max(1, N // 20))
        W = min(int(rng.choice([1, 3])), C)
        t = ib.build_ivf_index(xt, C=C, m=m, K=K, train_size=min(N, 4000), iters=3, seed=seed)
        pin = (t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
        ot = o.ivf_table(*pin)
        lists = pm.ivf_lists(o, ot, qs, k * pvf, W)
        pv = pm.expected(o, lists, vec_x, vec_ids, qs, k)
        an = aam.ivf_expected(o, ot, vec_x, vec_ids, triples, ka, n_cand, W)
        out.update(pin=pin, W=W, C=C)
        label += f" C={C} W={W} ka={ka}"
    else:
        t = ib.build_pq_index(xt, m=m, K=K, train_size=min(N, 4000), iters=3, seed=seed)
        pin = (t["codebook"], t["ids"], t["codes"])
        ot = o.pq_table(*pin)
        lists = pm.pq_lists(o, ot, qs, k * pvf)
        pv = pm.expected(o, lists, vec_x, vec_ids, qs, k)
        an = aam.pq_expected(o, ot, vec_x, vec_ids, triples, ka, n_cand)
        # the subset: known ids with and without a vector, some twice, unknown ones; a (k, pvf) of its own
        sub = rng.permutation(np.concatenate([ids[rng.choice(N, size=min(N, int(rng.choice([40, 600, 6000]))), replace=False)], missing[:5],
                                              ids[:7], [-5, 0, 10 ** 8]])).astype(np.int32)
        k2, pvf2 = PV_POOL[int(rng.integers(0, len(PV_POOL) - 1))]
        lists2 = pm.pq_lists(o, ot, qs, k2 * pvf2, sub)
        pv2 = pm.expected(o, lists2, vec_x, vec_ids, qs, k2)
        tg = rng.permutation(np.concatenate([ids[rng.choice(N, size=min(N, 300), replace=False)], [0, -3, 10 ** 8]])).astype(np.int32)
        sent = float(rng.choice([1000.0, 1.0]))
        out.update(pin=pin, subset=sub, k2=k2, pvf2=pvf2, pv2={"exp": pv2[0], "candidates": pv2[1], "scored": pv2[2], "lists": lists2},
                   assign_targets=tg, assign_sentinel=sent, assign_exp=asm.pq_assign(o, t["codebook"], t["ids"], t["codes"], qs, tg, sentinel=sent))
        label += f" ka={ka} subset={sub.size} k2={k2} pvf2={pvf2} assign_sentinel={sent}"
    out.update(label=label, pv={"exp": pv[0], "candidates": pv[1], "scored": pv[2], "lists": lists},
               analogy={"exp": an[0], "stats": an[1], "lists": an[2], "valid": an[4]})
    return out


# =======================================================================================
# mutation: one walk of ten steps per handle kind and seed
# =======================================================================================
MUTATION_SIZES = (1, 63, 64, 65, 300)
MUTATION_STEPS = 10
MUTATION_SPARE = 3000
REFUSALS = {"pq": ("dup_update", "code_K", "append_low"), "ivf": ("dup_update", "code_K", "cell_C", "append_low"),
            "ivpq": ("dup_update", "code_K", "cell_C", "append_low"), "vec": ("dup_update", "append_low")}
IVPQ_JOIN = (5, 3, 20, 2)        # (k, alpha, pvf, method) of the walk's join


def _mutation_rows(kind):
    """every row a walk may hold, in source order: {"x", "codes", "cell"} (what the kind has) and the tables that never change"""
    import test_gpu_mutation as tm
    if kind == "pq":
        cb, _, codes, x = tm._pq_source(300, 12, 256)
        return {"x": x, "codes": codes, "cell": None}, {"codebook": cb}
    if kind == "ivf":
        coarse, cb, _, cell, codes, x = tm._ivf_source(300, 12, 256, 32)
        return {"x": x, "codes": codes, "cell": cell}, {"coarse": coarse, "codebook": cb}
    if kind == "ivpq":
        t, x = tm._ivpq_source(True)
        return {"x": np.asarray(t["vectors"]), "codes": t["codes"], "cell": t["coarse_id"]}, {"codebook": t["codebook"], "coarse": t["coarse"], "stats": t["stats"]}
    x, _ = tm._vec_table(300, 9000)
    return {"x": x, "codes": None, "cell": None}, {}


def mutation_model(kind, start):
    """a fresh model of the walk's first state"""
    f, ids, p = start["fixed"], start["ids"], start["payload"]
    if kind == "pq":
        return um.PQModel(f["codebook"], ids, p["codes"])
    if kind == "ivf":
        return um.IVFModel.from_rows(f["coarse"], f["codebook"], ids, p["coarse_id"], p["codes"])
    if kind == "ivpq":
        return um.IVPQModel(f["codebook"], f["coarse"], ids, p["coarse_id"], p["codes"], p["vectors"], f["stats"])
    return um.VecModel(ids, p["vectors"])


def _payload_args(kind, p):
    """a payload dict -> the positional arguments the kind's model takes after the ids"""
    return {"pq": (p["codes"],), "ivf": (p["coarse_id"], p["codes"]), "ivpq": (p["coarse_id"], p["codes"], p["vectors"]), "vec": (p["vectors"],)}[kind]


def apply_to_model(kind, model, step):
    """one step on the model -> what the call returns (rows gone / changed, None otherwise); a refused step raises um.Refused"""
    op = step["call"]
    if op == "append":
        return model.append(step["ids"], *_payload_args(kind, step["payload"]))
    if op == "remove":
        return model.remove(step["ids"])
    if op == "update":
        return model.update(step["ids"], *_payload_args(kind, step["payload"]))
    return model.update_codebook(step["codebook"])


def model_ids(kind, model):
    return np.sort(np.concatenate(model.list_ids)) if kind == "ivf" else model.ids


def model_max_id(kind, model):
    if kind == "ivf":
        return model.max_id
    return int(model.ids[-1]) if model.N else -1


def model_bytes(kind, model):
    """every table of the model as bytes: two models are in the same state iff these are equal"""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in model.pin_args() if a is not None)


def mutation_lists(kind, o, model, qs, targets=None):
    """the oracle's answer to the walk's search on the model's tables (ivpq: (lists, iterations))"""
    ot = model.oracle_table(o)
    if kind == "pq":
        return np.stack([o.pq_search(ot, q, 7) for q in qs])
    if kind == "ivf":
        return o.ivfadc_search_many(ot, qs, 5, 3)
    if kind == "ivpq":
        k, alpha, pvf, method = IVPQ_JOIN
        return o.ivpq_search_in(ot, qs, k, targets, alpha, pvf, method)
    return [o.exact_knn(ot[0], ot[1], q, 5) for q in qs]


def _lists_ids(kind, lists):
    if kind == "ivpq":
        return lists[0]["id"].copy()
    if kind == "vec":
        return np.stack([np.pad(e["id"], (0, 5 - len(e)), constant_values=-1) for e in lists])
    return lists["id"].copy()


def draw_mutation(kind, seed, oracle=None):
    """Ten steps on one handle: append (A), remove (R), update (U), codebook swap (C; not for vec), each of a size from
    MUTATION_SIZES; one of the ten is a call the model refuses.  The first R or U of a walk names the nearest rows of four of the
    walk's queries, so that some step changes the answers."""
    import test_gpu_mutation as tm
    o = the_oracle(oracle)
    rng = np.random.default_rng(BASE["mutation"] + 100 * MUTATION_KINDS.index(kind) + seed)
    rows, fixed = _mutation_rows(kind)
    n0 = int(rng.integers(3000, 5001))
    total = rows["x"].shape[0]
    assert total >= n0 + MUTATION_SPARE
    spare = np.arange(n0, n0 + MUTATION_SPARE)

    def payload(r):
        r = np.asarray(r)
        return {"coarse_id": None if rows["cell"] is None else np.ascontiguousarray(rows["cell"][r], np.int32),
                "codes": None if rows["codes"] is None else np.ascontiguousarray(rows["codes"][r], np.int16),
                "vectors": np.ascontiguousarray(rows["x"][r], np.float32) if kind in ("ivpq", "vec") else None}

    ids0 = gapped_ids(rng, n0)
    start = {"fixed": fixed, "ids": ids0, "payload": payload(np.arange(n0))}
    model = mutation_model(kind, start)
    qrows = np.concatenate([rng.choice(n0, size=8, replace=False), rng.choice(spare, size=4, replace=False)])
    qs = np.ascontiguousarray(rows["x"][qrows], np.float32)
    ever = set(ids0.tolist())
    removed = []
    never = np.setdiff1d(ids0.astype(np.int64) + 1, ids0)[:400]          # ids in the gaps of the first state: no step brings them
    never = np.concatenate([never, [10 ** 8 + 1, 10 ** 8 + 3]])
    appended = []

    def targets():
        t = np.concatenate([ids0[::7], np.asarray(appended, np.int64)[::2], np.asarray(removed, np.int64)[:50], ids0[:20], [10 ** 8, -4]])
        return t.astype(np.int32)

    def lists():
        return mutation_lists(kind, o, model, qs, targets() if kind == "ivpq" else None)

    def id_mix(size, unique):
        """size ids from pinned U removed-earlier U never-known, shuffled (remove: a few of them twice)"""
        now = model_ids(kind, model)
        n_rem = min(len(removed), max(0, size // 6))
        n_nev = max(0, size // 6)
        n_now = max(1, size - n_rem - n_nev)
        parts = [rng.choice(now, size=min(n_now, now.size), replace=False),
                 rng.choice(np.asarray(removed, np.int64), size=n_rem, replace=False) if n_rem else np.empty(0, np.int64),
                 rng.choice(never, size=min(n_nev, never.size), replace=False)]
        out = np.unique(np.concatenate([np.asarray(p, np.int64) for p in parts]))
        if not unique and out.size > 3:
            out = np.concatenate([out, out[:2]])
        return rng.permutation(out)

    ops = "ARU" if kind == "vec" else "ARUC"
    refuse_at = int(rng.integers(1, MUTATION_STEPS))
    reason = REFUSALS[kind][int(rng.integers(0, len(REFUSALS[kind])))]
    last = MUTATION_STEPS - 1 if refuse_at != MUTATION_STEPS - 1 else MUTATION_STEPS - 2
    full_at = set(int(v) for v in rng.choice([s for s in range(MUTATION_STEPS) if s not in (refuse_at, last)], size=3, replace=False)) | {last}
    steps, first_ru = [], True
    before = _lists_ids(kind, lists())
    take = 0
    for si in range(MUTATION_STEPS):
        size = int(rng.choice(MUTATION_SIZES))
        if si == refuse_at:
            now = model_ids(kind, model)
            two = rng.choice(now, size=2, replace=False).astype(np.int32)
            if reason == "append_low":
                step = {"op": "refused", "reason": reason, "call": "append", "ids": np.array([model_max_id(kind, model)], np.int32), "payload": payload(spare[:1])}
            else:
                p = payload(spare[:3])
                ask = np.array([two[0], two[1], two[0]], np.int32) if reason == "dup_update" else np.array([two[0], two[1], never[0]], np.int32)
                if reason == "code_K":
                    p["codes"][1, -1] = model.K
                if reason == "cell_C":
                    p["coarse_id"][2] = model.C if kind == "ivf" else model.cells
                step = {"op": "refused", "reason": reason, "call": "update", "ids": ask, "payload": p}
            was = model_bytes(kind, model)
            try:
                apply_to_model(kind, model, step)
                raise AssertionError(f"the model took the step that is to be refused ({reason})")
            except um.Refused:
                pass
            assert model_bytes(kind, model) == was
            step.update(size=int(step["ids"].size), returns=None, bites=False)
        else:
            op = ops[int(rng.integers(0, len(ops)))]
            if op == "A":
                new = (model_max_id(kind, model) + np.cumsum(rng.integers(1, 3, size=size))).astype(np.int32)
                src = spare[(take + np.arange(size)) % spare.size]
                take += size
                step = {"op": "A", "call": "append", "ids": new, "payload": payload(src)}
                appended.extend(new.tolist())
                ever.update(new.tolist())
            elif op == "C":
                step = {"op": "C", "call": "codebook", "codebook": tm._nudged(model.codebook, 1000 * seed + si)}
            else:
                ask = id_mix(size, unique=op == "U")
                if first_ru:                       # the nearest rows of four queries: their answers change
                    near = np.unique(before[:4, 0])
                    ask = np.concatenate([ask[~np.isin(ask, near)], near[near >= 0]])
                    first_ru = False
                if op == "R":
                    step = {"op": "R", "call": "remove", "ids": ask.astype(np.int32)}
                else:
                    p = payload(rng.choice(spare, size=ask.size))
                    if kind == "ivf":              # the rows that exist change their cell where the drawn one is their own
                        own = model.cell_of(ask.astype(np.int32))
                        same = (own == p["coarse_id"]) & (own >= 0)
                        p["coarse_id"][same] = (own[same] + 1) % model.C
                    step = {"op": "U", "call": "update", "ids": ask.astype(np.int32), "payload": p}
            if op in "RU":
                step["names_removed"] = int(np.isin(step["ids"], np.asarray(removed, np.int64)).sum())
            if op == "U" and kind == "ivf":
                own = model.cell_of(step["ids"])
                step["cells_changed"] = int(((own >= 0) & (own != step["payload"]["coarse_id"])).sum())
            if op == "R":
                gone = np.intersect1d(model_ids(kind, model), step["ids"])
            step["returns"] = apply_to_model(kind, model, step)
            if op == "R":
                removed.extend(gone.tolist())
            step["size"] = size
        step["targets"] = targets() if kind == "ivpq" else None
        step["exp"] = lists()
        now_ids = _lists_ids(kind, step["exp"])
        step["bites"] = not np.array_equal(before, now_ids)
        before = now_ids
        step["full"] = si in full_at
        step["N"] = int(model.N)
        steps.append(step)
    label = (f"mutation kind={kind} seed={seed} n0={n0} refused={refuse_at}:{reason} full={sorted(full_at)} steps="
             + ",".join(f"{s['op'] if s['op'] != 'refused' else 'x'}{s['size'] if s['op'] != 'C' else ''}" for s in steps))
    return {"label": label, "kind": kind, "start": start, "qs": qs, "steps": steps, "final_bytes": model_bytes(kind, model), "n0": n0}
