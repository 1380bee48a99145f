"""GPU-box helper: the kNN-join (freddy_gpu_knn_join) with methods 0 (ADC) and 1 (exact) at k in {256, 512, 513, 1024, 2048,
4096} on the tables of bench.py --config join (1 M x 300, m = 30, K = 32, 32 x 32 cells), 256 queries x 100 000 targets,
alpha = ALPHA (3).  Up to k = 512 one workgroup per query selects 2k keys and replays them (join_query_kernel<V>); beyond that
join_query_kernel<16, true> selects 1024 keys per pass and bigk_replay_kernel writes the lists (csrc/bigk.h).
  1. k = 256 and k = 512, the path this change must not move: ms per call, medians of REPS.  The same lines come out of the parent
     commit's library (FREDDY_GPU_SO=<its libfreddy_gpu.so>; the tool sees that k = 513 is refused and stops after part 1), so the
     A/B is "run this tool with both libraries on ONE box, alternately" -- boxes differ by +-5 %.  Every run APPENDS part 1, marked
     "this" or "parent", to the log named by JOIN_BIGK_AB (default profiles/join_bigk_ab.txt): that file is never truncated.
  2. every k: ms per call, the HIP-event time between the first join launch and the end of the round (freddy_track's
     join_kernel_time, summed over the rounds) split into the join kernels' and the replay's share (replay_us), rounds, rows.
Writes profiles/join_bigk_timing.txt (join_bigk_timing_parent.txt with the parent's library) anew; PARTS=1 stops after part 1
and only appends to the A/B log (the repeated turns of the A/B; the committed join_bigk_timing.txt ends with that log).  N / Q /
REPS / ALPHA from the environment for a smaller run; JOIN_BIGK_TABLES names an .npz the tables are kept in between runs (built
when missing)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib   # noqa: E402

N, Q, T = int(os.environ.get("N", 1000000)), int(os.environ.get("Q", 256)), 100000
REPS, ALPHA, PARTS = int(os.environ.get("REPS", 7)), int(os.environ.get("ALPHA", 3)), int(os.environ.get("PARTS", 2))
KS = (256, 512, 513, 1024, 2048, 4096)
NAMES = ("codebook", "coarse", "ids", "coarse_id", "codes", "vectors", "stats")


def tables():
    path = os.environ.get("JOIN_BIGK_TABLES")
    if path and os.path.exists(path):
        z = np.load(path)
        return {n: z[n] for n in NAMES}
    import torch
    x = ib.make_corpus(N, d=300, seed=5, device=torch.device("cuda", 0))
    t = ib.build_ivpq_index(x, m=30, K=32, k_coarse=32, train_size=100000, iters=6, seed=3)
    t = {n: np.asarray(t[n]) for n in NAMES}
    if path:
        np.savez(path, **t)
    return t


t0 = time.time()
t = tables()
index = gpu.IVPQIndex(*[t[n] for n in NAMES])
rng = np.random.default_rng(4)
qs = t["vectors"][rng.choice(N, Q, replace=False)]
targets = rng.choice(np.arange(1, N + 1), T, replace=False).astype(np.int32)
try:
    index.knn_join(qs[:2], 513, targets, ALPHA, 1, 0)
    HAVE = True
except gpu.FreddyGpuError:
    HAVE = False
SIDE = "this  " if HAVE else "parent"
out = open(os.path.join(ROOT, "profiles", "join_bigk_timing.txt" if HAVE else "join_bigk_timing_parent.txt") if PARTS > 1 else os.devnull, "w")
ab = open(os.environ.get("JOIN_BIGK_AB", os.path.join(ROOT, "profiles", "join_bigk_ab.txt")), "a")


def say(line, ab_too=False):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()
    if ab_too:
        ab.write(f"{SIDE}: {line}\n")
        ab.flush()


def measure(method, k):
    """-> (median ms per call, the last call's track)"""
    for _ in range(2):
        index.knn_join(qs, k, targets, ALPHA, 1, method)
    ts = []
    for _ in range(REPS):
        t1 = time.perf_counter()
        index.knn_join(qs, k, targets, ALPHA, 1, method)
        ts.append(time.perf_counter() - t1)
    return statistics.median(ts) * 1e3, index.last_track()


say(f"# kNN-join, {N} x 300, m=30 K=32 32x32 cells, {Q} queries x {T} targets, alpha={ALPHA}, medians of {REPS} (setup {time.time() - t0:.0f} s); "
    f"this library {'takes' if HAVE else 'REFUSES'} k > 512 with methods 0 / 1", ab_too=True)
say("# 1. the path up to k = 512")
say("# method    k   call_ms", ab_too=True)
part1 = {}
for method in (0, 1):
    for k in (256, 512):
        part1[(method, k)] = measure(method, k)
        say(f"{method:6d} {k:5d}  {part1[(method, k)][0]:8.3f}", ab_too=True)
if HAVE and PARTS > 1:
    say("# 2. every k: the events' time = join kernels + replay (summed over the rounds)")
    say("# method    k   call_ms  events_ms  join_kernels_ms  replay_ms  replay_share  rounds  candidate_rows")
    ms512 = {}
    for method in (0, 1):
        for k in KS:
            ms, tr = part1[(method, k)] if (method, k) in part1 else measure(method, k)
            ev, rp = tr["join_kernel_time"] * 1e3, tr.get("replay_us", 0) * 1e-3
            say(f"{method:6d} {k:5d}  {ms:8.3f}  {ev:9.3f}  {ev - rp:15.3f}  {rp:9.3f}  {rp / ev if ev > 0 else 0.0:12.3f}  {tr['iterations']:6d}  {tr['candidate_rows']:14d}")
            if k == 512:
                ms512[method] = (ms, ev)
            if k == 513:
                say(f"# method {method}: k = 513 over k = 512: call {ms / ms512[method][0]:.2f}x, events {ev / ms512[method][1]:.2f}x")
out.close()
ab.close()
index.close()
