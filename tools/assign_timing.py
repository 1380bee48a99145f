"""GPU-box helper: the assignment step of cluster_exact / cluster_pq (csrc/assign.h) on the bench tables (3 M x 300; flat PQ index
m = 12, K = 1024).
  1. cluster_exact / cluster_pq of the host mirror at n = 4096 tokens, k in {10, 100}, supplied draws: the time of one call
     (ten rounds), medians of REPS.  The same lines come out of a checkout of the parent commit (the tool runs there unchanged: it
     skips part 2 when the library has no assign entry points), so the A/B is "run this tool in both trees on ONE box, alternately"
     -- boxes differ by +-5 %, the comparison is not valid across boxes.  Every run APPENDS these lines, marked "this" or
     "parent", to the log named by ASSIGN_AB (default profiles/assign_ab.txt of the tree it runs in; give both trees the same
     path): that file is never truncated, it is the record of the A/B.
  2. the new path alone: one assign call and its kernel (the handle's profile) at n in {4096, 100 000, 3 000 000}, Q in {10, 100};
     the exact kernel's achieved bytes/s (n * d * 4 gathered per 16-query tile) and fp32 flop/s (2 * n * Q * d) against the HBM and
     VALU peaks of the MI355X (8 TB/s; 256 CUs x 128 lanes x 2.4 GHz x 1 separately rounded op = 78.6 Tflop/s without FMA).
Writes profiles/assign_timing.txt (assign_timing_parent.txt in a tree without the entry points) anew and appends part 1 to the A/B
log.  N / REPS from the environment for a smaller run.
ASSIGN_FILTER_AB=1: instead of the above, option assign_filter 0 and 1 ALTERNATED on one vector handle in one process, ROUNDS (3)
rounds: freddy_gpu_exact_assign at Q in {10, 100, 1000}, n in {4096, 100 000, 3 M}, and freddy_gpu_cluster (cluster_exact, ten rounds)
at kc in {10, 100} and the same n; equal outputs are asserted before anything is timed; per setting the kernels' time (the handle's
profile, all assign_ kernels) of every round, so the baseline's own spread stands beside the gain; candidates per target and the
redo count from freddy_gpu_last_assign_stats.  Writes profiles/assign_filter_timing.txt."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib, udf   # noqa: E402

N, REPS = int(os.environ.get("N", 3000000)), int(os.environ.get("REPS", 5))
D, HBM_PEAK, VALU_PEAK = 300, 8.0e12, 256 * 128 * 2.4e9
HAVE = hasattr(gpu.load(), "freddy_gpu_exact_assign")
FILTER_AB = bool(os.environ.get("ASSIGN_FILTER_AB"))
out = open(os.path.join(ROOT, "profiles", "assign_filter_timing.txt" if FILTER_AB else "assign_timing.txt" if HAVE else "assign_timing_parent.txt"), "w")
SIDE = "this  " if HAVE else "parent"


def say(line, ab_too=False):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()
    if ab_too:
        ab.write(f"{SIDE}: {line}\n")
        ab.flush()


def filter_ab():
    rounds = int(os.environ.get("ROUNDS", 3))
    xh = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0)).cpu().numpy()
    ids = np.arange(1, N + 1, dtype=np.int32)
    vec = gpu.VectorIndex(ids, xh)
    rng = np.random.default_rng(7)

    def kernel_ms(call, option):
        vec.set_option("assign_filter", option)
        vec.profile_enable(True)
        res = call()
        ms = sum(t for nm, (_, t) in vec.profile_read().items() if nm.startswith("assign_"))
        vec.profile_enable(False)
        return res, ms

    say(f"# option assign_filter 0 / 1 alternated on one handle, {N} x {D}, {rounds} rounds; kernel_ms = all assign_ kernels of one call")
    say("# call            n   Q/kc   off_ms (rounds)            on_ms (rounds)             off/on  cand/target  redone")
    for n in (4096, 100000, min(N, 3000000)):
        tg = rng.choice(ids, n).astype(np.int32)
        for what, sizes in (("exact_assign", (10, 100, 1000)), ("cluster_exact", (10, 100))):
            for Q in sizes:
                if what == "exact_assign":
                    cent = np.stack([xh[rng.choice(N, 10)].mean(axis=0) for _ in range(Q)]).astype(np.float32)
                    call = lambda: vec.assign(cent, tg)                                   # noqa: E731
                else:
                    draws = rng.random(Q + 9 * Q * 10)
                    call = lambda: vec.cluster(tg, Q, draws)                              # noqa: E731
                (a, _), (b, _) = kernel_ms(call, 0), kernel_ms(call, 1)                     # warm-up, and the outputs
                assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b)), (what, n, Q)
                off, on = [], []
                for _ in range(rounds):
                    off.append(kernel_ms(call, 0)[1])
                    on.append(kernel_ms(call, 1)[1])
                st = vec.last_assign_stats()
                fmt = lambda ts: " ".join(f"{t:8.3f}" for t in ts)                          # noqa: E731
                say(f"{what:14s} {n:8d} {Q:5d}   {fmt(off)}   {fmt(on)}   {statistics.median(off) / statistics.median(on):6.2f}"
                    f"  {st['candidates'] / max(st['filtered'], 1):11.2f}  {st['redone']:6d}")
    vec.close()


if FILTER_AB:
    filter_ab()
    out.close()
    sys.exit(0)
ab = open(os.environ.get("ASSIGN_AB", os.path.join(ROOT, "profiles", "assign_ab.txt")), "a")
t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
pq = ib.build_pq_index(x, m=12, K=1024, train_size=100000, iters=10, seed=2)
xh = x.cpu().numpy()
del x
ids = np.arange(1, N + 1, dtype=np.int32)
s = udf.Session()
s.load_vecs_norm(ids, xh)
s.load_pq(pq["codebook"], pq["ids"], pq["codes"])
rng = np.random.default_rng(7)
say(f"# assignment step, {N} x {D}, PQ m=12 K=1024, medians of {REPS} (setup {time.time() - t0:.0f} s); this tree {'has' if HAVE else 'has NOT'} the assign entry points", ab_too=True)
say("# 1. host mirror, n = 4096 tokens, ten rounds per call")
say("# function       k   call_ms")
tokens = np.sort(rng.choice(ids, 4096, replace=False)).astype(np.int32)
for name in ("cluster_exact", "cluster_pq"):
    for k in (10, 100):
        draws = rng.random(k + 9 * k * 10)
        getattr(s, name)(tokens, k, draws)     # warm-up (pins the vectors, sizes the workspaces)
        ts = []
        for _ in range(REPS):
            t = time.perf_counter(); getattr(s, name)(tokens, k, draws); ts.append(time.perf_counter() - t)
        say(f"{name:14s} {k:3d}  {statistics.median(ts) * 1e3:8.2f}", ab_too=True)
if HAVE:
    say("# 2. one assign call")
    say("# call            n        Q   call_ms  kernel_ms  gathered_GB/s  of_HBM_peak  Gflop/s  of_VALU_peak")
    for which, table in (("exact", "vecs"), ("pq", "pq")):
        idx = s.gpu_index(table)
        for n in (4096, 100000, min(N, 3000000)):
            tg = rng.choice(ids, n).astype(np.int32)
            for Q in (10, 100):
                cent = np.stack([xh[rng.choice(N, 10)].mean(axis=0) for _ in range(Q)]).astype(np.float32)
                call = (lambda: s.exact_assign(cent, tg)) if which == "exact" else (lambda: s.pq_assign(cent, tg))
                call()
                ts = []
                for _ in range(REPS):
                    t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
                idx.profile_enable(True)
                call()
                prof = idx.profile_read()
                idx.profile_enable(False)
                k_ms = sum(ms for nm, (_, ms) in prof.items() if nm.startswith("assign_"))
                line = f"{which + '_assign':14s} {n:8d} {Q:5d}  {statistics.median(ts) * 1e3:8.2f}  {k_ms:9.3f}"
                if which == "exact" and k_ms > 0:
                    by = n * D * 4 * ((Q + 15) // 16) / (k_ms * 1e-3)
                    fl = 2.0 * n * Q * D / (k_ms * 1e-3)
                    line += f"  {by / 1e9:13.1f}  {by / HBM_PEAK:11.4f}  {fl / 1e9:7.0f}  {fl / VALU_PEAK:12.4f}"
                say(line)
out.close()
ab.close()
