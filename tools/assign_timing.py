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
log.  N / REPS from the environment for a smaller run."""
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
out = open(os.path.join(ROOT, "profiles", "assign_timing.txt" if HAVE else "assign_timing_parent.txt"), "w")
ab = open(os.environ.get("ASSIGN_AB", os.path.join(ROOT, "profiles", "assign_ab.txt")), "a")
SIDE = "this  " if HAVE else "parent"


def say(line, ab_too=False):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()
    if ab_too:
        ab.write(f"{SIDE}: {line}\n")
        ab.flush()


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
