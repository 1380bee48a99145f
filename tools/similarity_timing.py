"""GPU-box helper: the similarities by row id (csrc/similarity.h) over the bench's vector table (3 M x 300), one MI355X.
  1. pairs: 1 / 1 024 / 100 000 / 10 M pairs per call -- the call, its kernel (the handle's profile), the gathered bytes per second
     (2 rows x 4 d bytes per pair) against the HBM peak; beside it what a caller pays today: the host's gather of both rows from its
     copy plus the oracle's chain on one core (one ctypes call per pair, up to 100 000 pairs -- 10 M are not run on the host).
  2. matrix: 100 x 3 M, 1 024 x 100 000, 4 096 x 4 096 (A by vectors) against freddy_gpu_exact_assign at the same (Q, n_targets) -- the
     same chains and the same staging, no result stream -- runs alternated; the kernels' ratio, the call's, and what the na * nb * 4
     bytes of the D2H copy cost by themselves (call minus kernels).
  3. join: the same shapes at thresholds that pass about 0, 0.1 % and 10 % of the pairs (quantiles of a sample of the matrix), against
     matrix + np.nonzero on the host; the count, scan and fill kernels beside the matrix kernel.
Writes profiles/similarity_timing.txt anew.  N / REPS from the environment for a smaller run."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib   # noqa: E402
from oracle.oracle import Oracle                # noqa: E402

N, REPS = int(os.environ.get("N", 3000000)), int(os.environ.get("REPS", 3))
D, HBM_PEAK, VALU_PEAK = 300, 8.0e12, 256 * 128 * 2.4e9
out = open(os.path.join(ROOT, "profiles", "similarity_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(call, reps=REPS):
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def profile(idx, call):
    idx.profile_enable(True)
    call()
    prof = idx.profile_read()
    idx.profile_enable(False)
    return {k: ms for k, (_, ms) in prof.items()}


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
xh = x.cpu().numpy()
del x
ids = np.arange(1, N + 1, dtype=np.int32)
vec = gpu.VectorIndex(ids, xh)
oracle = Oracle()
rng = np.random.default_rng(7)
say(f"# similarities by row id, {N} x {D}, medians of {REPS} (setup {time.time() - t0:.0f} s)")

say("# 1. pairs")
say("# pairs      call_ms  kernel_ms  gathered_GB/s  of_HBM_peak   host_ms  (host: numpy gather of both rows + the oracle's chain, one core)")
for n in (1, 1024, 100000, 10000000):
    a, b = rng.choice(ids, n).astype(np.int32), rng.choice(ids, n).astype(np.int32)
    call_ms = timed(lambda: vec.similarity_pairs(a, b))
    k_ms = profile(vec, lambda: vec.similarity_pairs(a, b)).get("sim_pairs_kernel", 0.0)
    by = 2.0 * n * D * 4 / (k_ms * 1e-3) if k_ms > 0 else 0.0
    host = "   not run"
    if n <= 100000:
        def host_pairs():
            va, vb = xh[a - 1], xh[b - 1]
            return [oracle.cosine_similarity_bytea(va[i], vb[i]) for i in range(n)]
        host = f"{timed(host_pairs, 1 if n > 1024 else REPS):10.3f}"
    say(f"{n:9d}  {call_ms:9.3f}  {k_ms:9.3f}  {by / 1e9:13.1f}  {by / HBM_PEAK:11.4f}  {host}")

say("# 2. matrix (A by vectors) against exact_assign at the same (Q = na, n_targets = nb), alternated")
say("#    na       nb  matrix_call_ms  matrix_kernel_ms  assign_call_ms  assign_kernel_ms  kernel_ratio  call_ratio  out_MB  call-kernels_ms  Gflop/s  of_VALU_peak")
SHAPES = [(100, min(N, 3000000)), (1024, min(N, 100000)), (4096, min(N, 4096))]
kept = {}
for na, nb in SHAPES:
    av = np.stack([xh[rng.choice(N, 4)].mean(axis=0) for _ in range(na)]).astype(np.float32)
    b = rng.choice(ids, nb, replace=False).astype(np.int32)
    vec.similarity_matrix(av, b); vec.assign(av, b)
    tm, ta = [], []
    for _ in range(REPS):
        t = time.perf_counter(); vec.assign(av, b); ta.append(time.perf_counter() - t)
        t = time.perf_counter(); res = vec.similarity_matrix(av, b); tm.append(time.perf_counter() - t)
    pm = profile(vec, lambda: vec.similarity_matrix(av, b))
    pa = profile(vec, lambda: vec.assign(av, b))
    km, ka = pm.get("sim_matrix_kernel", 0.0), pa.get("assign_exact_kernel", 0.0)
    m_ms, a_ms = statistics.median(tm) * 1e3, statistics.median(ta) * 1e3
    fl = 2.0 * na * nb * D / (km * 1e-3)
    say(f"{na:7d} {nb:8d}  {m_ms:14.2f}  {km:16.3f}  {a_ms:14.2f}  {ka:16.3f}  {km / ka:12.3f}  {m_ms / a_ms:10.2f}  {na * nb * 4 / 1e6:6.0f}  "
        f"{m_ms - sum(pm.values()):15.2f}  {fl / 1e9:7.0f}  {fl / VALU_PEAK:12.4f}")
    say("#         kernels of the matrix call: " + ", ".join(f"{k} {v:.3f} ms" for k, v in sorted(pm.items())))
    kept[(na, nb)] = (av, b, res[0])

say("# 3. join: the matrix's shapes, thresholds that pass about 0, 0.1 % and 10 % of the pairs; host = similarity_matrix + np.nonzero(out > t)")
say("#    na       nb  passing  pairs        join_call_ms  host_ms   matrix_kernel_ms  count_ms  scan_ms  fill_ms")
for (na, nb), (av, b, m) in kept.items():
    sample = m.ravel()[rng.integers(0, m.size, size=1000000)]
    for frac in (0.0, 0.001, 0.1):
        thr = np.float32(2.0) if frac == 0.0 else np.float32(np.quantile(sample, 1.0 - frac))
        total = vec.similarity_join(av, b, thr, max_pairs=0)[3]

        def host_join():
            o = vec.similarity_matrix(av, b)[0]
            return np.nonzero(o > thr)
        j_ms = timed(lambda: vec.similarity_join(av, b, thr, max_pairs=total), 1)
        h_ms = timed(host_join, 1)
        p = profile(vec, lambda: vec.similarity_join(av, b, thr, max_pairs=total))
        say(f"{na:7d} {nb:8d}  {frac:7.3f}  {total:11d}  {j_ms:12.2f}  {h_ms:7.2f}  {p.get('sim_matrix_kernel', 0):17.3f}  {p.get('sim_count_kernel', 0):8.3f}  "
            f"{p.get('sim_scan_kernel', 0):7.3f}  {p.get('sim_fill_kernel', 0):7.3f}")
vec.close()
out.close()
