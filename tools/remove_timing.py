"""GPU-box helper: one freddy_gpu_remove_rows call against what the glue does today for a DELETE -- unpin, and pin the remaining
rows again -- on the bench index (3 M x 300, C = 1000, m = 12, K = 1024) and on the 3 M x 300 vector table, removing 1, 1 000 and
100 000 random rows.  The re-pin is the same code in the parent commit and in this tree, so both sides of the comparison run in
one process on one box.  Then the cost of the arrangement a compacted list loses: a batch of 1024 queries (nprobe 10, k 5, the
shape of bench.py's step) on a fresh pin, on the handle after a tenth of its rows has been removed, and on a fresh pin of those
remaining rows -- call time and the scan kernel's time from the handle's profile.
Writes profiles/remove_timing.txt anew.  N / REPS from the environment for a smaller run."""
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
C, M, K, D = int(os.environ.get("C", 1000)), 12, 1024, 300
out = open(os.path.join(ROOT, "profiles", "remove_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def remaining(t, cell, gone):
    keep = ~np.isin(t["ids"], gone)
    lo = np.zeros(C + 1, np.int32)
    lo[1:] = np.cumsum(np.bincount(cell[keep], minlength=C))
    return t["coarse"], t["codebook"], lo, t["ids"][keep], t["codes"][keep]


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
t = ib.build_ivf_index(x, C=C, m=M, K=K, train_size=min(N, 100000), iters=10, seed=1)
xh = x.cpu().numpy()
del x
cell = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)
vec_ids = np.arange(1, N + 1, dtype=np.int32)
rng = np.random.default_rng(11)
say(f"# remove_rows against unpin + pin of the remaining rows, {N} x {D}, C={C} m={M} K={K}, one call each (setup {time.time() - t0:.0f} s)")
say("# handle   removed   remove_ms   unpin_pin_ms   ratio")
for n in (1, 1000, 100000):
    if n >= N:
        continue
    gone = rng.choice(t["ids"], n, replace=False).astype(np.int32)
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    got, ms = timed(lambda: idx.remove_rows(gone))
    assert got == n
    args = remaining(t, cell, gone)          # (host work the glue does either way: not timed)
    _, ms_pin = timed(lambda: (idx.close(), gpu.IVFIndex(*args))[1].close())
    say(f"ivf     {n:8d}  {ms:10.2f}  {ms_pin:13.2f}  {ms_pin / ms:6.1f}")
for n in (1, 1000, 100000):
    if n >= N:
        continue
    gone = rng.choice(vec_ids, n, replace=False).astype(np.int32)
    idx = gpu.VectorIndex(vec_ids, xh)
    got, ms = timed(lambda: idx.remove_rows(gone))
    assert got == n
    keep = ~np.isin(vec_ids, gone)
    ids2, x2 = vec_ids[keep], xh[keep]
    _, ms_pin = timed(lambda: (idx.close(), gpu.VectorIndex(ids2, x2))[1].close())
    del x2
    say(f"vectors {n:8d}  {ms:10.2f}  {ms_pin:13.2f}  {ms_pin / ms:6.1f}")

say("# a batch of 1024 queries, nprobe 10, k 5: medians of %d calls; scan = the scan kernel's time in the handle's profile" % REPS)
say("# handle                                  call_ms   scan_ms")
qs = np.ascontiguousarray(xh[rng.choice(N, 1024, replace=False)])
gone = rng.choice(t["ids"], N // 10, replace=False).astype(np.int32)


def batch(idx, what):
    idx.search(qs, 5, 10)
    ts = [timed(lambda: idx.search(qs, 5, 10))[1] for _ in range(REPS)]
    idx.profile_enable(True)
    idx.search(qs, 5, 10)
    prof = idx.profile_read()
    idx.profile_enable(False)
    scan = sum(ms for nm, (_, ms) in prof.items() if nm in ("ivf_filter", "sparse_items"))
    say(f"{what:38s} {statistics.median(ts):8.3f}  {scan:8.3f}")


idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
batch(idx, "fresh pin, all rows")
idx.remove_rows(gone)
batch(idx, "after remove_rows of a tenth")
idx.close()
idx = gpu.IVFIndex(*remaining(t, cell, gone))
batch(idx, "fresh pin of the remaining rows")
idx.close()
out.close()
