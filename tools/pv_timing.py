"""GPU-box helper: post verification on the bench workload (3 M x 300, C = 1000, m = 12, K = 1024, W = 10, k = 5, 1024 queries).
For pvf in {1, 2, 4, 6, 20}: recall@5 against the exact kNN, the time of one freddy_gpu_ivfadc_search_pv call, the pv_ kernels' share
of it (the handle's profile) and their achieved bytes/s (scored * d * 4 over kernel time) against the HBM peak -- beside the only
thing the library offered before: the host mirror's k_nearest_neighbour_ivfadc_pv (ivfadc_search at k * pvf, then the host loop
of knn_pv) called once per query.  The two are timed alternately, REPS times each, medians reported.
Writes profiles/pv_timing.txt.  N / Q / REPS from the environment for a smaller run."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib, udf   # noqa: E402

N, Q, REPS = int(os.environ.get("N", 3000000)), int(os.environ.get("Q", 1024)), int(os.environ.get("REPS", 5))
K, W, HBM_PEAK = 5, 10, 8.0e12
dev = torch.device("cuda", 0)
out = open(os.path.join(ROOT, "profiles", "pv_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=dev)
tab = ib.build_ivf_index(x, C=1000, m=12, K=1024, train_size=100000, iters=10, seed=2)
rng = np.random.default_rng(7)
qids = np.sort(rng.choice(np.arange(1, N + 1), size=Q, replace=False)).astype(np.int64)
q = x[torch.from_numpy(qids - 1).to(dev)].contiguous()
exact = ib.exact_topk(x, q, K)
qs, xh = q.cpu().numpy(), x.cpu().numpy()
del x
ids = np.arange(1, N + 1, dtype=np.int32)
ivf = gpu.IVFIndex(tab["coarse"], tab["codebook"], tab["list_off"], tab["ids"], tab["codes"])
vec = gpu.VectorIndex(ids, xh)
s = udf.Session()
s.load_vecs_norm(ids, xh)
s.load_ivfadc(tab["coarse"], tab["codebook"], tab["ids"], np.repeat(np.arange(1000), np.diff(tab["list_off"])).astype(np.int32), tab["codes"])
s.set_w(W)
say(f"# post verification, {N} x 300, C=1000 m=12 K=1024 W={W} k={K}, {Q} queries, medians of {REPS} alternating repetitions (setup {time.time() - t0:.0f} s)")
say("# pvf  recall@5  device_call_ms  pv_kernels_ms  pv_share  scored  pv_GB/s  of_HBM_peak  host_per_query_loop_ms  speedup")
for pvf in (1, 2, 4, 6, 20):
    s.set_pvf(pvf)
    gi, _ = ivf.search_pv(vec, qs, K, pvf, W)                      # warm-up (buffers, the vector handle's first use)
    s.k_nearest_neighbour_ivfadc_pv(qs[0], K)
    recall = ib.recall_at_k(gi, exact)
    t_dev, t_host = [], []
    for _ in range(REPS):
        t = time.perf_counter(); ivf.search_pv(vec, qs, K, pvf, W); t_dev.append(time.perf_counter() - t)
        t = time.perf_counter()
        for i in range(Q):
            s.k_nearest_neighbour_ivfadc_pv(qs[i], K)
        t_host.append(time.perf_counter() - t)
    ivf.profile_enable(True)
    ivf.search_pv(vec, qs, K, pvf, W)
    prof = ivf.profile_read()
    ivf.profile_enable(False)
    pv_ms = sum(ms for name, (_, ms) in prof.items() if name.startswith("pv_"))
    all_ms = sum(ms for _, ms in prof.values())
    scored = ivf.last_pv_stats()["scored"]
    bps = scored * 300 * 4 / (pv_ms * 1e-3) if pv_ms > 0 else 0.0
    d_ms, h_ms = statistics.median(t_dev) * 1e3, statistics.median(t_host) * 1e3
    say(f"{pvf:5d}  {recall:8.4f}  {d_ms:14.3f}  {pv_ms:13.4f}  {pv_ms / all_ms if all_ms else 0:8.3f}  {scored:6d}  {bps / 1e9:7.1f}  {bps / HBM_PEAK:11.4f}  {h_ms:22.1f}  {h_ms / d_ms:7.1f}")
    say(f"#        kernels: " + ", ".join(f"{n} {ms:.3f} ms" for n, (_, ms) in sorted(prof.items())))
out.close()
