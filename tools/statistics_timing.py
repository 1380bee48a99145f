"""GPU-box helper: the statistics row of a pinned ivpq handle on the bench tables (3 M x 300; ivpq m = 30, K = 32, k_coarse = 8,
pinned with vectors) -- freddy_gpu_create_statistics over every pinned row, over 100 000 and over 10 M ids (drawn with
replacement: a column has duplicates), and freddy_gpu_set_statistics; for comparison the host's way to the same row
(np.bincount over the host copy of the cells, the model's arithmetic, then set_statistics) and the only way there was before:
unpin, and pin again with the new row.  Every figure is the median of REPS calls after one call that is reported on its own
(the first call of a size allocates the pinned staging block).
Writes profiles/statistics_timing.txt anew.  N / REPS from the environment for a smaller run."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib   # noqa: E402

N, REPS = int(os.environ.get("N", 3000000)), int(os.environ.get("REPS", 5))
D = 300
out = open(os.path.join(ROOT, "profiles", "statistics_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


def row(what, f):
    _, first = timed(f)
    ms = statistics.median(timed(f)[1] for _ in range(REPS))
    say(f"{what:58s} {first:10.3f}  {ms:10.3f}")
    return ms


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
tj = ib.build_ivpq_index(x, m=30, K=32, k_coarse=8, train_size=min(N, 100000), iters=4, seed=3, keep_vectors=False)
xh = x.cpu().numpy()
del x
rng = np.random.default_rng(12)
cells = tj["coarse"].shape[1] ** 2
pin = lambda stats: gpu.IVPQIndex(tj["codebook"], tj["coarse"], tj["ids"], tj["coarse_id"], tj["codes"], xh, stats)


def host_row(cell):
    count = np.bincount(cell, minlength=cells)
    r = np.empty(cells + 1, np.float32)
    r[:cells] = (count.astype(np.float64) / np.float64(cell.size)).astype(np.float32)
    r[cells] = np.float32(cell.size)
    return r


say(f"# the statistics row of a pinned ivpq handle, {N} x {D}, {cells} cells (setup {time.time() - t0:.0f} s)")
say(f"# {'call':56s}   first_ms   median_ms   (median of {REPS})")
idx = pin(tj["stats"])
got, matched = idx.create_statistics()
assert matched == N and np.array_equal(got.view(np.uint32), host_row(tj["coarse_id"]).view(np.uint32))
row("create_statistics, every pinned row", lambda: idx.create_statistics())
for n in (100000, 10000000):
    col = tj["ids"][rng.integers(0, N, n)]
    got, matched = idx.create_statistics(col)
    assert matched == n and np.array_equal(got.view(np.uint32), host_row(tj["coarse_id"][col - 1]).view(np.uint32))
    row(f"create_statistics, {n} ids", lambda: idx.create_statistics(col))
    row(f"create_statistics, {n} ids, installed", lambda: idx.create_statistics(col, install=True))
other = host_row(tj["coarse_id"][: N // 2])
row("set_statistics", lambda: idx.set_statistics(other))
row("host: np.bincount over the cells + set_statistics", lambda: idx.set_statistics(host_row(tj["coarse_id"])))
state = {"idx": idx}


def repin():
    state["idx"].close()
    state["idx"] = pin(other)


row("unpin + pin with the new row", repin)
state["idx"].close()
out.close()
