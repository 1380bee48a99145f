"""GPU-box helper: the kNN-join by row id (freddy_gpu_knn_join_ids) and the batched analogy over the kNN-join (freddy_gpu_ivpq_analogy) on
the tables of `bench.py --config join` (1 M x 300, m = 30, K = 32, 2 x 32 coarse codes; k = 5, alpha = 100, pvf = 20, method 2).
Per Q in {64, 1024, 5000} x 100 000 targets, a new target array every call, six variants alternated within ONE process over several
rounds:
  ids      knn_join_ids(vector handle, query ids)           4 bytes per query go up, sub_dist_rows_kernel gathers
  ids_own  knn_join_ids(None, query ids)                    the same from the ivpq handle's own vectors
  gather0  ids with option join_front_gather = 0            query_gather_kernel, then sub_dist_kernel
  host     knn_join(pageable floats)                        the float entry point, unchanged by this work
  pinned   knn_join(a PinnedBuffer)
  today    knn_join(xh[rows]): the host's gather + host     what a caller that starts from ids pays without the new call
then the join_front_rows kernel's time from the handle's profile with the bytes it moves set against the HBM peak, and the analogy:
1024 triples per call at n_cand = 4 against the loop of single analogy_3cosadd_in_ivpq calls (the host mirror) and against
freddy_gpu_pq_analogy over the same subset, with the share of answers equal to the exact analogy_3cosadd_in.
Writes profiles/join_ids_timing.txt: per figure the median of every round's calls, the medians over the rounds, and the spread
(max - min) / median of the baseline's (host) own rounds -- a difference inside it is no difference.
  join_ids_timing.py            N / ROUNDS / REPS_S (seconds of calls per figure and round) / TRIPLES from the environment for a smaller run"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROUNDS, REPS_S = int(os.environ.get("N", 1000000)), int(os.environ.get("ROUNDS", 5)), float(os.environ.get("REPS_S", 0.12))
TRIPLES = int(os.environ.get("TRIPLES", 1024))
K, D, T, ALPHA, PVF, METHOD, HBM_PEAK = 5, 300, 100000, 100, 20, 2, 8.0e12
JOIN_Q = (64, 1024, 5000)


def main():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu, index_build as ib, udf
    gpu.load()
    note = lambda what: print(f"[join_ids_timing] {what}", file=sys.stderr, flush=True)
    note("building the tables")
    dev = torch.device("cuda", 0)
    x = ib.make_corpus(N, d=D, seed=5, device=dev)
    t = ib.build_ivpq_index(x, m=30, K=32, k_coarse=32, train_size=min(N, 100000), iters=6, seed=3)
    pq = ib.build_pq_index(x, m=12, K=256, train_size=min(N, 100000), iters=6, seed=2)
    del x
    torch.cuda.empty_cache()
    xh = t["vectors"]
    ids = t["ids"]
    index = gpu.IVPQIndex(t["codebook"], t["coarse"], ids, t["coarse_id"], t["codes"], xh, t["stats"])
    vec = gpu.VectorIndex(ids, xh)
    rng = np.random.default_rng(4)
    qid = rng.choice(ids, max(JOIN_Q), replace=False).astype(np.int32)
    hq = np.ascontiguousarray(xh[qid - 1])
    targets = [rng.choice(ids, min(T, N), replace=False).astype(np.int32) for _ in range(7)]   # taken in turn: no call repeats its predecessor's array
    n_call = [0]

    def tg():
        n_call[0] += 1
        return targets[n_call[0] % len(targets)]

    def timed(call):
        call()
        t0 = time.perf_counter(); call(); one = time.perf_counter() - t0
        ts = [one]
        for _ in range(int(min(200, max(2, REPS_S / max(one, 1e-6))))):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)   # (every call is synchronous)
        return statistics.median(ts) * 1e3

    def gather0(call):
        def run():
            index.set_option("join_front_gather", 0)
            try:
                return timed(call)
            finally:
                index.set_option("join_front_gather", 1)
        return run

    def variants(Q, pb):
        q, qi = hq[:Q], qid[:Q]
        pb.array[:Q] = q
        join = lambda qs: index.knn_join(qs, K, tg(), ALPHA, PVF, METHOD)
        by_ids = lambda v: index.knn_join_ids(v, qi, K, tg(), ALPHA, PVF, METHOD)
        return {"ids": lambda: timed(lambda: by_ids(vec)), "ids_own": lambda: timed(lambda: by_ids(None)), "gather0": gather0(lambda: by_ids(vec)),
                "host": lambda: timed(lambda: join(q)), "pinned": lambda: timed(lambda: join(pb.array[:Q])), "today": lambda: timed(lambda: join(xh[qi - 1]))}

    def rounds_of(vs):
        res = {n: [] for n in vs}
        for _ in range(ROUNDS):
            for n, f in vs.items():
                res[n].append(f())
        return res

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = open(os.path.join(ROOT, "profiles", "join_ids_timing.txt"), "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    fmt = lambda v: "/".join(f"{a:.3f}" for a in v)
    names = ("ids", "ids_own", "gather0", "host", "pinned", "today")
    say(f"# kNN-join by row id, {N} x {D}, {min(T, N)} targets (a new array every call), k = {K}, alpha = {ALPHA}, pvf = {PVF}, method {METHOD}; ms per call: the median of")
    say(f"# each round's calls, {ROUNDS} rounds, one process, the variants alternated inside every round.  spread: (max - min) / median of host's own rounds.")
    say("#     Q  " + " ".join(f"{n:>9s}" for n in names) + "   spread  ids/today  ids/host  ids/pinned  same lists   rounds: ids | host | today")
    pb = gpu.PinnedBuffer((max(JOIN_Q), D))
    for Q in JOIN_Q:
        note(f"join Q = {Q}")
        r = rounds_of(variants(Q, pb))
        m = {n: med(v) for n, v in r.items()}
        one = targets[0]
        a = index.knn_join_ids(vec, qid[:Q], K, one, ALPHA, PVF, METHOD)
        b = index.knn_join(hq[:Q], K, one, ALPHA, PVF, METHOD)
        ok = bool(np.array_equal(a[1], b[0]) and np.array_equal(a[2].view(np.uint32), b[1].view(np.uint32)) and a[3] == b[2])
        sp = spread(r["host"])
        say(f"{Q:7d}  " + " ".join(f"{m[n]:9.3f}" for n in names) + f"   {sp:6.3f}  {m['ids'] / m['today']:9.3f}  {m['ids'] / m['host']:8.3f}  {m['ids'] / m['pinned']:10.3f}  "
            f"{str(ok):10s}   {fmt(r['ids'])} | {fmt(r['host'])} | {fmt(r['today'])}")
        slower = m["ids"] > m["today"] * (1.0 + sp)
        say(f"#   Q = {Q}: ids {m['ids']:.3f} ms against today's path {m['today']:.3f} ms ({(1.0 - m['ids'] / m['today']) * 100:.1f} % less; host's spread {sp * 100:.1f} %)"
            f"{' -- SLOWER than today beyond the spread' if slower else ''}")
    pb.close()
    say()
    say("# the front kernel (the handle's profile: device events), per call; bytes: a row read and written (8 d), the sub-distances written (8 Kc) and the row")
    say("# number read (4) per query -- the multi-index centroids (4 d Kc bytes, shared by every workgroup) are not counted")
    say("#     Q  join_front_rows us    bytes      GB/s   of the HBM peak (8 TB/s)   |  join_front_gather = 0: query_gather us")
    Kc = t["coarse"].shape[1]
    for Q in JOIN_Q:
        us = {}
        for g in (1, 0):
            index.set_option("join_front_gather", g)
            index.profile_enable(True)
            for _ in range(5):
                index.knn_join_ids(vec, qid[:Q], K, tg(), ALPHA, PVF, METHOD)
            prof = index.profile_read()
            index.profile_enable(False)
            us[g] = prof.get("join_front_rows" if g else "query_gather", (0, 0.0))[1] * 1e3 / 5
        index.set_option("join_front_gather", 1)
        moved = Q * (8 * D + 8 * Kc + 4)
        say(f"{Q:7d}  {us[1]:18.2f}  {moved:9d}  {moved / (us[1] * 1e-6) / 1e9:8.1f}   {moved / (us[1] * 1e-6) / HBM_PEAK:8.4f}{'':20s}|  {us[0]:8.2f}")
    say()

    # ---- the analogy ----
    note("analogy")
    tr = rng.choice(ids, (TRIPLES, 3)).astype(np.int32)
    sub = targets[0]
    pqi = gpu.PQIndex(pq["codebook"], pq["ids"], pq["codes"])
    s = udf.Session()
    s.load_vecs_norm(ids, xh)
    s.load_ivpq(t["codebook"], t["coarse"], ids, t["coarse_id"], t["codes"], t["stats"])
    s.set_alpha(ALPHA); s.set_pvf(PVF); s.set_method_flag(METHOD)
    res = {n: [] for n in ("batch", "mirror_batch", "loop", "pq_batch")}
    n_loop = min(TRIPLES, 256)
    for _ in range(ROUNDS):
        res["batch"].append(timed(lambda: index.analogy(vec, tr, 1, 4, target_ids=sub, alpha=ALPHA, pvf=PVF, method=METHOD)))
        res["mirror_batch"].append(timed(lambda: s.analogy_3cosadd_in_ivpq_batch(tr, sub)))
        t0 = time.perf_counter()
        loop = [s.analogy_3cosadd_in_ivpq(int(a), int(b), int(c), sub) for a, b, c in tr[:n_loop]]
        res["loop"].append((time.perf_counter() - t0) * 1e3 * TRIPLES / n_loop)
        res["pq_batch"].append(timed(lambda: pqi.analogy(vec, tr, 1, PVF + 3, sentinel=1000.0, subset_ids=sub)))
    batch = s.analogy_3cosadd_in_ivpq_batch(tr, sub)
    same_as_loop = bool(np.array_equal(batch[:n_loop], np.array(loop, np.int32)))
    pq_ans = pqi.analogy(vec, tr, 1, PVF + 3, sentinel=1000.0, subset_ids=sub)[0][:, 0]
    n_exact = min(TRIPLES, 256)
    exact = np.array([s.analogy_3cosadd_in(int(a), int(b), int(c), sub) for a, b, c in tr[:n_exact]], np.int32)
    m = {n: med(v) for n, v in res.items()}
    say(f"# analogy_3cosadd_in_ivpq for {TRIPLES} triples per call over the same {sub.size} targets (alpha = {ALPHA}, pvf = {PVF}, method {METHOD}; the SQL's literal n_cand = 4); ms per call")
    say(f"# loop: single analogy_3cosadd_in_ivpq calls of the host mirror, timed over {n_loop} triples and scaled to {TRIPLES}; pq_batch: freddy_gpu_pq_analogy, n_cand = pvf + 3")
    say(f"#   batch (freddy_gpu_ivpq_analogy) {m['batch']:9.3f}   mirror batch {m['mirror_batch']:9.3f}   loop {m['loop']:9.3f}   pq_batch {m['pq_batch']:9.3f}"
        f"   loop/batch {m['loop'] / m['mirror_batch']:7.1f}   rounds: {fmt(res['batch'])} | {fmt(res['loop'])}")
    say(f"#   the batch answers as the loop does: {same_as_loop};  answers equal to the exact analogy_3cosadd_in (first {n_exact} triples): "
        f"ivpq {float((batch[:n_exact] == exact).mean()):.3f}, pq {float((pq_ans[:n_exact] == exact).mean()):.3f}")
    out.close()
    s.close()
    for h in (index, vec, pqi):
        h.close()


if __name__ == "__main__":
    main()
