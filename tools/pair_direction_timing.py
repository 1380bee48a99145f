"""GPU-box helper: analogy_pair_direction (analogy.h) at 3 M x 300, k = 1, through the host-buffer ABI -- ms per call and
analogies per second at 1, 32 and 1024 analogies per call, beside the yardstick: 3CosAdd with exact_filter = 0 (the all-exact
scan, the nearest existing kernel) on the same table and call sizes.  End-to-end figures come from a host clock around calls
that end in a device synchronise, profiler off, after a warm-up call of the same shape, windows of at least ~1 s; the per-kernel
split comes from a second pass with the library's own HIP-event profiler on.  One spot check against the numpy model.
Writes profiles/pair_direction_timing.txt (or the path given as the first argument)."""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu, index_build as ib
import pair_model as pm

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pair_direction_timing.txt")
N = int(os.environ.get("PAIR_N", 3_000_000))
assert torch.cuda.is_available(), "this tool measures on the GPU"
dev = torch.device("cuda", 0)
x = ib.make_corpus(N, seed=11, device=dev).cpu().numpy()
x *= np.random.default_rng(5).uniform(0.5, 4.0, size=(N, 1)).astype(np.float32)   # the original table is not normalised
ids = np.arange(1, N + 1, dtype=np.int32)
d = x.shape[1]
idx = gpu.VectorIndex(ids, x)
idx.set_option("exact_filter", 0)            # the yardstick is the all-exact scan; pair direction has no other path
rng = np.random.default_rng(0)
triples = ids[rng.integers(0, N, size=(1024, 3))]
# lane-instructions per (row, analogy) counted from the kernel's inner loops: sweep 1 sub, mul, add; sweep 2 sub, division (~10), mul, add
est_instr = d * (3 + 13)
out = {"N": N, "d": d, "k": 1, "row_bytes": N * d * 4, "est_lane_instr_per_row_analogy": est_instr}
lines = []
for method in ("pair_direction", "3cosadd"):
    for Q in (1, 32, 1024):
        t0 = time.perf_counter()
        gi, gs = idx.analogy(triples[:Q], k=1, method=method)      # warm-up of this shape (and a first estimate of its time)
        first = time.perf_counter() - t0
        n = max(3, min(200, int(1.0 / max(first, 1e-4))))
        times = []
        for _ in range(3):                                           # three windows: the spread shows beside the median
            t0 = time.perf_counter()
            for _ in range(n):
                idx.analogy(triples[:Q], k=1, method=method)
            times.append((time.perf_counter() - t0) / n)
        dt = sorted(times)[1]
        idx.profile_enable(True)                                     # the split, in a pass of its own
        np_ = max(1, n // 4)
        for _ in range(np_):
            idx.analogy(triples[:Q], k=1, method=method)
        prof = idx.profile_read()
        idx.profile_enable(False)
        rec = {"ms_per_call": round(dt * 1e3, 3), "ms_per_call_min_max": [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
               "calls_per_window": n, "analogies_per_s": round(Q / dt, 1),
               "kernels_ms_per_call": {k: round(v[1] / np_, 3) for k, v in sorted(prof.items())},
               "kernel_launches_per_call": {k: v[0] // np_ for k, v in sorted(prof.items())},
               "filter_passes": idx.last_analogy_stats()["filter_passes"]}
        scan = prof.get("analogy_pair_scan" if method == "pair_direction" else "analogy_scan")
        if scan:
            ms = scan[1] / np_
            tiles = (Q + 7) // 8 if Q > 8 else 1                     # workgroup tiles of analogies, each loading the table per sweep
            sweeps = 2 if method == "pair_direction" else 1
            rec["scan_table_loads"] = tiles * sweeps
            rec["scan_row_load_TBps"] = round(N * d * 4 * tiles * sweeps / (ms * 1e-3) / 1e12, 3)
            if method == "pair_direction":
                rec["scan_lane_instr_per_s"] = round(est_instr * N * Q / (ms * 1e-3), 0)
        out[f"{method}_Q{Q}"] = rec
        if method == "pair_direction" and Q == 1024:
            keep = (gi, gs)
        lines.append(f"{method} {Q} {json.dumps(rec)}")
        print(lines[-1], flush=True)
# spot check: one analogy of the 1024-call against the numpy model (id and score bits)
t0 = time.perf_counter()
ei, es = pm.model(x, ids, triples[777:778], 1)
out["check_777"] = {"parity": bool(ei[0, 0] == keep[0][777, 0] and es[0, 0].view(np.uint64) == keep[1][777, 0].view(np.uint64)),
                    "cpu_numpy_s_per_analogy": round(time.perf_counter() - t0, 2)}
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n" + json.dumps(out, indent=1) + "\n")
print(json.dumps(out["check_777"]))
