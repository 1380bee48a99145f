"""GPU-box helper: the exact kNN-join and exact kNN by row id (freddy_gpu_exact_join_ids / freddy_gpu_exact_search_ids, id sets resolved
on the device: csrc/resolve.h) on 3 M x 300, ids 1 .. N, k = 5.  Per shape four variants of the join, alternated within ONE process
over several rounds (the baseline is the unchanged entry point of the same build, option exact_resolve = 0: the parent's code path):
  ids     exact_join_ids(query ids, target ids)              queries gathered and targets resolved on the device
  host0   exact_join(vectors, target ids), exact_resolve = 0  the baseline: the host resolves the targets
  host1   the same with exact_resolve = 1                      host vectors, targets resolved on the device
  today   exact_join(xh[rows], ...), exact_resolve = 0         what a caller that starts from ids pays today: the host's gather + host0
at Q x targets in {64, 1024, 5000} x {1000, 8000, 100000, N}; exact_search_ids against exact_search at Q in {1, 64} over the whole
table and over a 100 000-id subset; the 5000 x 100000 and 64 x 1000 joins again after 3000 rows spread over the table were removed
(ids with gaps); and the three stages of the resolve from the handle's profile (device events) with the bytes they move set against
the HBM peak.  Writes profiles/exact_ids_timing.txt: per figure the median of every round's calls, the medians over the rounds, and
the spread (max - min) / median of the baseline's own rounds -- a difference inside it is no difference.
  exact_ids_timing.py            N / ROUNDS / REPS_S (seconds of calls per figure and round) from the environment for a smaller run"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROUNDS, REPS_S = int(os.environ.get("N", 3000000)), int(os.environ.get("ROUNDS", 5)), float(os.environ.get("REPS_S", 0.12))
K, D, HBM_PEAK = 5, 300, 8.0e12
JOIN_Q, JOIN_T = (64, 1024, 5000), (1000, 8000, 100000, N)


def main():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
    from freddy_amd import gpu, index_build as ib
    gpu.load()
    note = lambda what: print(f"[exact_ids_timing] {what}", file=sys.stderr, flush=True)
    note("building the table")
    xh = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0)).cpu().numpy()
    torch.cuda.empty_cache()
    ids = np.arange(1, N + 1, dtype=np.int32)
    rng = np.random.default_rng(7)
    qid = rng.choice(ids, size=max(JOIN_Q), replace=False).astype(np.int32)
    hq = np.ascontiguousarray(xh[qid - 1])
    tid = {T: (rng.choice(ids, size=T, replace=False).astype(np.int32) if T < N else rng.permutation(ids).astype(np.int32)) for T in JOIN_T}
    vec = gpu.VectorIndex(ids, xh)
    POS = gpu.QIDS_POSITIONAL

    def timed(call):
        call()
        t = time.perf_counter(); call(); one = time.perf_counter() - t
        ts = [one]
        for _ in range(int(min(200, max(2, REPS_S / max(one, 1e-6))))):
            t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)   # (every call is synchronous)
        return statistics.median(ts) * 1e3

    def with_resolve(v, call):
        def run():
            vec.set_option("exact_resolve", v)
            try:
                return timed(call)
            finally:
                vec.set_option("exact_resolve", 0)
        return run

    def join_variants(Q, T):
        q, qi, t = hq[:Q], qid[:Q], tid[T]
        return {"ids": lambda: timed(lambda: vec.exact_join_ids(qi, K, t, rule=POS)),
                "host0": with_resolve(0, lambda: vec.join(q, K, t)),
                "host1": with_resolve(1, lambda: vec.join(q, K, t)),
                "today": with_resolve(0, lambda: vec.join(xh[qi - 1], K, t))}

    def search_variants(Q, sub):
        q, qi = hq[:Q], qid[:Q]
        return {"ids": lambda: timed(lambda: vec.exact_search_ids(qi, K, subset_ids=sub, rule=POS)),
                "host0": with_resolve(0, lambda: vec.search(q, K, subset_ids=sub)),
                "host1": with_resolve(1, lambda: vec.search(q, K, subset_ids=sub))}

    def rounds_of(variants):
        """variant -> [median ms of each round], the variants alternated inside every round"""
        res = {n: [] for n in variants}
        for _ in range(ROUNDS):
            for n, f in variants.items():
                res[n].append(f())
        return res

    def same(a, b):
        return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))

    out = open(os.path.join(ROOT, "profiles", "exact_ids_timing.txt"), "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")

    fmt = lambda v: "/".join(f"{t:.3f}" for t in v)
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    say(f"# exact kNN-join / exact kNN by row id, {N} x {D}, ids 1 .. N, k = {K}; ms per call: the median of each round's calls, {ROUNDS} rounds, one process,")
    say("# the variants alternated inside every round.  spread: (max - min) / median of host0's own rounds.")
    say("# ids: exact_join_ids   host0: exact_join, exact_resolve = 0 (baseline)   host1: exact_join, exact_resolve = 1   today: host gather of the query rows + host0")
    say(f"#     Q  targets   {'ids':>9s} {'host0':>9s} {'host1':>9s} {'today':>9s}   spread  ids/host0  ids/today  host1/host0  same lists   rounds: ids | host0")
    verdict = {}
    for T in JOIN_T:
        for Q in JOIN_Q:
            note(f"join Q = {Q}, targets = {T}")
            r = rounds_of(join_variants(Q, T))
            m = {n: med(v) for n, v in r.items()}
            ok = same(vec.exact_join_ids(qid[:Q], K, tid[T], rule=POS)[1:], vec.join(hq[:Q], K, tid[T]))
            say(f"{Q:7d} {T:8d}   {m['ids']:9.3f} {m['host0']:9.3f} {m['host1']:9.3f} {m['today']:9.3f}   {spread(r['host0']):6.3f}  {m['ids'] / m['host0']:9.3f}  "
                f"{m['ids'] / m['today']:9.3f}  {m['host1'] / m['host0']:11.3f}  {str(ok):10s}   {fmt(r['ids'])} | {fmt(r['host0'])}")
            verdict[(Q, T)] = (m, spread(r["host0"]))
    if (5000, 100000) in verdict:
        m, sp = verdict[(5000, 100000)]
        gain = 1.0 - m["ids"] / m["today"]
        say(f"# acceptance, 5000 x 100000: exact_join_ids {m['ids']:.3f} ms against today's path {m['today']:.3f} ms: {gain * 100:.1f} % less, the baseline's spread is "
            f"{sp * 100:.1f} % -> {'faster by more than the spread' if gain > sp else 'NOT faster by more than the spread'}")
    say()
    say("# exact_search_ids against exact_search: the whole table, and a subset of 100 000 ids")
    say(f"#     Q  subset    {'ids':>9s} {'host0':>9s} {'host1':>9s}   spread  ids/host0  same lists")
    sub = tid[100000] if 100000 in tid else tid[JOIN_T[0]]
    for s, what in ((None, "-"), (sub, str(sub.size))):
        for Q in (1, 64):
            note(f"search Q = {Q}, subset = {what}")
            r = rounds_of(search_variants(Q, s))
            m = {n: med(v) for n, v in r.items()}
            ok = same(vec.exact_search_ids(qid[:Q], K, subset_ids=s, rule=POS)[1:], vec.search(hq[:Q], K, subset_ids=s))
            say(f"{Q:7d} {what:>8s}   {m['ids']:9.3f} {m['host0']:9.3f} {m['host1']:9.3f}   {spread(r['host0']):6.3f}  {m['ids'] / m['host0']:9.3f}  {ok}")
    say()
    say("# the three stages of the resolve (the handle's profile: device events, five calls of debug_resolve_ids), per call; bytes: the bitmap cleared once and")
    say("# read twice (3 N / 8), 4 n ids read, 4 nT rows written (the mark kernel's atomics and its lookups of the id array are not counted)")
    say("#        n   mark us   scan us  place us   total us    bytes      GB/s   of the HBM peak (8 TB/s)   resolve_block")
    for B in (0, 64):
        vec.set_option("resolve_block", B)
        for T in JOIN_T:
            vec.profile_enable(True)
            for _ in range(5):
                vec.debug_resolve_ids(tid[T])
            prof = vec.profile_read()
            vec.profile_enable(False)
            us = [prof.get(n, (0, 0.0))[1] * 1e3 / 5 for n in ("resolve_mark", "resolve_scan", "resolve_place")]
            moved = 3 * (N // 8) + 8 * T
            say(f"{T:10d}  {us[0]:8.2f}  {us[1]:8.2f}  {us[2]:8.2f}   {sum(us):8.2f}  {moved:10d}  {moved / (sum(us) * 1e-6) / 1e9:8.1f}   {moved / (sum(us) * 1e-6) / HBM_PEAK:8.4f}"
                f"{'':20s}{B if B else 256}")
    vec.set_option("resolve_block", 0)
    say()
    say("# ids with gaps: 3000 rows spread over the table removed from the handle (no query id among them)")
    say(f"#     Q  targets   {'ids':>9s} {'host0':>9s}   spread  ids/host0  same lists")
    gone = np.setdiff1d(ids[::max(N // 3000, 1)], qid).astype(np.int32)
    vec.remove_rows(gone)
    for Q, T in ((64, 1000), (5000, 100000)):
        if T not in tid:
            continue
        v = join_variants(Q, T)
        r = rounds_of({n: v[n] for n in ("ids", "host0")})
        m = {n: med(x) for n, x in r.items()}
        ok = same(vec.exact_join_ids(qid[:Q], K, tid[T], rule=POS)[1:], vec.join(hq[:Q], K, tid[T]))
        say(f"{Q:7d} {T:8d}   {m['ids']:9.3f} {m['host0']:9.3f}   {spread(r['host0']):6.3f}  {m['ids'] / m['host0']:9.3f}  {ok}")
    out.close()
    vec.close()


if __name__ == "__main__":
    main()
