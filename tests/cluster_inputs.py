"""The steered cases of tests/test_gpu_cluster.py, built without a device (tests/test_cluster_inputs_cpu.py proves on the CPU what
their traces reach).  The draws are the handle: membership after round 1 depends only on draws[0:kc], so a case computes the first
assignment with the model and then sets the round-1 draws of a cluster to r = (x - 0.5) / len for the ranks x it wants (pick(len, r)
= rint(x - 0.5 + 0.5) = x).  Two equal initial draws give two identical centroids, of which the later never wins: the empty cluster."""
import functools

import numpy as np

import assign_model as am
import cluster_model as cm
import util

N = 20000
SHAPES = {"300d_m12": (300, 12, 256), "25d_m5": (25, 5, 256)}
STEP = 8 * 256          # csrc/cluster.h: positions per step of cluster_sample_kernel's walk (CL_SUB * CL_WG)


@functools.lru_cache(maxsize=None)
def tables(shape):
    """The 20 000-row tables of tests/test_gpu_assign.py: (x, ids, codebook, codes)."""
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


def run_model(case, oracle=None):
    x, ids, cb, codes = tables(case["shape"])
    if case["method"] == "exact":
        return cm.exact(ids, x, case["tokens"], case["kc"], case["draws"], case["rounds"])
    return cm.pq(oracle, ids, x, cb, ids, codes, case["tokens"], case["kc"], case["draws"], case["rounds"], sentinel=case["sentinel"])


def _first_assignment(case):
    """(best[n], members per cluster) of round 1 of an exact case."""
    x, ids, _, _ = tables(case["shape"])
    vec = cm.token_vectors(ids, x, case["tokens"])
    cent = np.stack([vec[cm.pick(vec.shape[0], case["draws"][i]) - 1] for i in range(case["kc"])])
    best, _ = am.exact_assign(ids, x, cent, case["tokens"])
    return best, [np.flatnonzero(best == i) for i in range(case["kc"])]


def _steer(case, wanted):
    """wanted: {cluster: [rank, ...]} -> the round-1 draws of those clusters, in the order given (the other draws stay random)."""
    _, members = _first_assignment(case)
    kc = case["kc"]
    for i, ranks in wanted.items():
        assert len(ranks) <= cm.SAMPLES
        ln = members[i].size
        for t, x in enumerate(ranks):
            assert 1 <= x <= ln
            case["draws"][kc + i * cm.SAMPLES + t] = (x - 0.5) / ln
            assert cm.pick(ln, case["draws"][kc + i * cm.SAMPLES + t]) == x
    return case


def _case(name, shape, method, n, kc, rounds, seed, sentinel=1000.0):
    _, ids, _, _ = tables(shape)
    rng = np.random.default_rng(seed)
    tokens = rng.choice(ids, n).astype(np.int32)          # unsorted, with repeats
    return dict(name=name, shape=shape, method=method, tokens=tokens, kc=kc, rounds=rounds, draws=rng.random(cm.n_draws(kc, rounds)),
                sentinel=sentinel)


def _rank_of(members, pos):
    return int(np.searchsorted(members, pos)) + 1


@functools.lru_cache(maxsize=None)
def steered_cases():
    cases = []
    # ranks at the ends, across a wave and across 256 positions, a member drawn twice, an empty cluster in front of sampling ones
    c = _case("ranks", "25d_m5", "exact", 1000, 5, 3, 101)
    c["tokens"][64] = c["tokens"][63]; c["tokens"][256] = c["tokens"][255]      # the same id: the same cluster
    c["draws"][1] = c["draws"][0]                                               # cluster 1 repeats cluster 0's centroid: it stays empty
    best, members = _first_assignment(c)
    assert members[1].size == 0 and best[63] == best[64] and best[255] == best[256]
    wanted = {}
    for p in (63, 64, 255, 256):
        wanted.setdefault(int(best[p]), []).append(_rank_of(members[best[p]], p))
    big = max((i for i in range(5) if i not in wanted), key=lambda i: members[i].size)
    wanted[big] = [1, members[big].size, 1]
    cases.append(_steer(c, wanted))
    # the same across a step of the sample kernel's walk
    c = _case("step", "25d_m5", "exact", STEP + 452, 3, 2, 102)
    c["tokens"][STEP] = c["tokens"][STEP - 1]
    best, members = _first_assignment(c)
    i = int(best[STEP])
    cases.append(_steer(c, {i: [_rank_of(members[i], STEP - 1), _rank_of(members[i], STEP), members[i].size, 1]}))
    cases.append(_case("kc_above_n", "25d_m5", "exact", 3, 5, 3, 103))
    cases.append(_case("kc_1", "25d_m5", "exact", 257, 1, 3, 104))
    # a sentinel that leaves tokens unclaimed: stale members (|members| > lens) and positions that end in cluster 0
    cases.append(_case("unclaimed", "25d_m5", "pq", 300, 4, 4, 105, sentinel=UNCLAIMED_SENTINEL))
    return cases


UNCLAIMED_SENTINEL = 0.5


def reached(case, out):
    """What the trace of one case reaches (section (b) of the issue), as a set of names."""
    got = set()
    tr = [r for r in out["trace"] if r[2] >= 0]
    by = {}
    for J, i, t, x, ln, pos in tr:
        by.setdefault((J, i), []).append(pos)
        if x == 1: got.add("rank_1")
        if x == ln: got.add("rank_len")
    for (J, i), ps in by.items():
        s = set(p for p in ps if p >= 0)
        if any(p % 64 == 63 and p + 1 in s for p in s): got.add("wave_edge")
        if any(p % 256 == 255 and p + 1 in s for p in s): got.add("chunk_edge")
        if any(p % STEP == STEP - 1 and p + 1 in s for p in s): got.add("step_edge")
        if len([p for p in ps if p >= 0]) > len(s): got.add("drawn_twice")
    skipped = [(J, i) for J, i, t, *_ in out["trace"] if t < 0]
    if any((J, j) in by for J, i in skipped for j in range(i + 1, case["kc"])): got.add("empty_before_sampling")
    if any(m > ln for _, _, m, ln in out["members"]): got.add("stale_member")
    if (out["clusters"] == 0).any(): got.add("cluster_0")
    if case["kc"] > case["tokens"].size: got.add("kc_above_n")
    if case["kc"] == 1: got.add("kc_1")
    return got


WANTED = {"rank_1", "rank_len", "wave_edge", "chunk_edge", "step_edge", "drawn_twice", "empty_before_sampling", "stale_member", "cluster_0",
          "kc_above_n", "kc_1"}
