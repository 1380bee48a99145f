"""GPU-box helper: exact analogies (analogy.h) at 3 M x 300 through the host-buffer ABI -- analogies per second for
Q in {1, 32, 1024, 19544} and both methods, per-kernel HIP-event times from the library's own profiler, candidates per analogy
and passes redone on the all-exact path (freddy_gpu_last_analogy_stats), the filter pass's bytes / time against HBM peak, two spot checks against the numpy model with a CPU figure beside the GPU one."""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu, index_build as ib
import analogy_model as am

N = int(os.environ.get("ANALOGY_N", 3_000_000))
HBM_PEAK = 8.0e12            # MI355X, bytes/s
dev = torch.device("cuda", 0)
x = ib.make_corpus(N, seed=11, device=dev).cpu().numpy()
ids = np.arange(1, N + 1, dtype=np.int32)
t0 = time.perf_counter()
idx = gpu.VectorIndex(ids, x)
d = x.shape[1]
out = {"N": N, "d": d, "pin_s": round(time.perf_counter() - t0, 2)}
filter_bytes = (N + 31) // 32 * ((d + 15) // 16) * 2 * 64 * 16   # the fragment copy one filter pass streams
rng = np.random.default_rng(0)
triples = ids[rng.integers(0, N, size=(19544, 3))]
res = {}
for method in ("3cosmul", "3cosadd"):
    for Q in (1, 32, 1024, 19544):
        idx.analogy(triples[:Q], k=1, method=method)
        idx.profile_enable(True)
        n = 3 if Q <= 1024 else 1
        t0 = time.perf_counter()
        for _ in range(n):
            gi, gs = idx.analogy(triples[:Q], k=1, method=method)
        dt = (time.perf_counter() - t0) / n
        prof = idx.profile_read()
        idx.profile_enable(False)
        st = idx.last_analogy_stats()
        f = prof.get("analogy_filter")
        rec = {"ms_per_call": round(dt * 1e3, 3), "analogies_per_s": round(Q / dt, 1),
               "kernels_us": {k: round(v[1] / v[0] * 1e3, 1) for k, v in prof.items()},
               "kernels_ms_per_call": {k: round(v[1] / n, 3) for k, v in prof.items()},
               "filter_passes": st["filter_passes"], "redone_passes": st["redone_passes"],
               "candidates_per_analogy": round(st["candidates"] / Q, 1)}
        if f:
            per = f[1] / f[0] * 1e-3
            rec["filter_pass_TBps"] = round(filter_bytes / per / 1e12, 2)
            rec["filter_pass_frac_hbm_peak"] = round(filter_bytes / per / HBM_PEAK, 3)
        out[f"{method}_Q{Q}"] = rec
        res[(method, Q)] = (gi, gs)
        print(method, Q, json.dumps(rec), flush=True)
# spot checks: two analogies per method against the numpy model (ids and score bits), with the CPU time of the model
x_t = np.ascontiguousarray(x.T)
for method in ("3cosmul", "3cosadd"):
    gi, gs = res[(method, 1024)]
    for q in (0, 777):
        t0 = time.perf_counter()
        ei, es = am.model(x, ids, triples[q:q + 1], 1, method, x_t=x_t)
        cpu = time.perf_counter() - t0
        out[f"check_{method}_{q}"] = {"parity": bool(ei[0, 0] == gi[q, 0] and es[0, 0].view(np.uint64) == gs[q, 0].view(np.uint64)),
                                      "cpu_numpy_s_per_analogy": round(cpu, 2),
                                      "gpu_s_per_analogy_Q1024": round(out[f"{method}_Q1024"]["ms_per_call"] / 1024 / 1e3, 6)}
out["bound_violations"] = idx.bound_violations()
print(json.dumps(out, indent=1))
