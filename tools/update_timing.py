"""GPU-box helper: one freddy_gpu_update_rows call against the only way the parent commit reaches the same state -- unpin, and pin
the updated table again -- on the bench tables (3 M x 300; ivf C = 1000, m = 12, K = 1024; pq m = 12, K = 1024; ivpq m = 30,
K = 32 with vectors; the vector table), updating 1, 100 and 10 000 random rows.  For ivf half of the rows change their cell.
The re-pin is the same code in the parent commit and in this tree, so both sides of the comparison run in one process on one
box.  Then the cost of the arrangement the lists lose: a batch of 1024 queries (nprobe 10, k 5, the shape of bench.py's step)
before and after the 10 000-row update, and on a fresh pin of the updated table -- call time and the scan kernel's time from
the handle's profile.
Writes profiles/update_timing.txt anew.  N / REPS / KINDS from the environment for a smaller run."""
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
KINDS = os.environ.get("KINDS", "ivf,pq,ivpq,vectors").split(",")
C, M, K, D = int(os.environ.get("C", 1000)), 12, 1024, 300
SIZES = (1, 100, 10000)
out = open(os.path.join(ROOT, "profiles", "update_timing.txt"), "w")


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


def ivf_lists(t, ids, cell, codes):
    """rows in any order -> the arguments of a pin: lists ordered by id"""
    order = np.lexsort((ids, cell))
    lo = np.zeros(C + 1, np.int32)
    lo[1:] = np.cumsum(np.bincount(cell, minlength=C))
    return t["coarse"], t["codebook"], lo, ids[order], codes[order]


def row(kind, n, ms, ms_pin):
    say(f"{kind:8s}{n:8d}  {ms:10.2f}  {ms_pin:13.2f}  {ms_pin / ms:7.1f}")


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
t = ib.build_ivf_index(x, C=C, m=M, K=K, train_size=min(N, 100000), iters=10, seed=1) if "ivf" in KINDS else None
tp = ib.build_pq_index(x, m=M, K=K, train_size=min(N, 100000), iters=4, seed=2) if "pq" in KINDS else None
tj = ib.build_ivpq_index(x, m=30, K=32, k_coarse=8, train_size=min(N, 100000), iters=4, seed=3, keep_vectors=False) if "ivpq" in KINDS else None
xh = x.cpu().numpy()
del x
rng = np.random.default_rng(12)
say(f"# update_rows against unpin + pin of the updated table, {N} x {D}, one call each (setup {time.time() - t0:.0f} s)")
say("# handle  updated   update_ms   unpin_pin_ms    ratio")
sizes = [n for n in SIZES if n < N]

if t is not None:
    cell = np.repeat(np.arange(C), np.diff(t["list_off"])).astype(np.int32)

    def ivf_payload(n):
        """n random rows get the codes of n other rows; every second one also that row's cell (or the next cell, if it is its own)"""
        at = rng.choice(N, n, replace=False)
        donor = rng.choice(N, n, replace=False)
        new_cell = cell[at].copy()
        new_cell[::2] = np.where(cell[donor[::2]] == cell[at[::2]], (cell[at[::2]] + 1) % C, cell[donor[::2]])
        return at, new_cell.astype(np.int32), t["codes"][donor]

    for n in sizes:
        at, new_cell, new_codes = ivf_payload(n)
        idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
        got, ms = timed(lambda: idx.update_rows(t["ids"][at], coarse_id=new_cell, codes=new_codes))
        assert got == n
        cell2, codes2 = cell.copy(), t["codes"].copy()
        cell2[at], codes2[at] = new_cell, new_codes
        args = ivf_lists(t, t["ids"], cell2, codes2)          # (host work the glue does either way: not timed)
        _, ms_pin = timed(lambda: (idx.close(), gpu.IVFIndex(*args))[1].close())
        row("ivf", n, ms, ms_pin)
if tp is not None:
    for n in sizes:
        at, donor = rng.choice(N, n, replace=False), rng.choice(N, n, replace=False)
        idx = gpu.PQIndex(tp["codebook"], tp["ids"], tp["codes"])
        got, ms = timed(lambda: idx.update_rows(tp["ids"][at], codes=tp["codes"][donor]))
        assert got == n
        codes2 = tp["codes"].copy(); codes2[at] = tp["codes"][donor]
        _, ms_pin = timed(lambda: (idx.close(), gpu.PQIndex(tp["codebook"], tp["ids"], codes2))[1].close())
        row("pq", n, ms, ms_pin)
if tj is not None:
    pin = lambda cid, codes, vec: gpu.IVPQIndex(tj["codebook"], tj["coarse"], tj["ids"], cid, codes, vec, tj["stats"])
    for n in sizes:
        at, donor = rng.choice(N, n, replace=False), rng.choice(N, n, replace=False)
        idx = pin(tj["coarse_id"], tj["codes"], xh)
        got, ms = timed(lambda: idx.update_rows(tj["ids"][at], coarse_id=tj["coarse_id"][donor], codes=tj["codes"][donor], vectors=xh[donor]))
        assert got == n
        cid2, codes2, x2 = tj["coarse_id"].copy(), tj["codes"].copy(), xh.copy()
        cid2[at], codes2[at], x2[at] = tj["coarse_id"][donor], tj["codes"][donor], xh[donor]
        _, ms_pin = timed(lambda: (idx.close(), pin(cid2, codes2, x2))[1].close())
        del x2
        row("ivpq", n, ms, ms_pin)
if "vectors" in KINDS:
    vec_ids = np.arange(1, N + 1, dtype=np.int32)
    for n in sizes:
        at, donor = rng.choice(N, n, replace=False), rng.choice(N, n, replace=False)
        idx = gpu.VectorIndex(vec_ids, xh)
        got, ms = timed(lambda: idx.update_rows(vec_ids[at], vectors=xh[donor]))
        assert got == n
        x2 = xh.copy(); x2[at] = xh[donor]
        _, ms_pin = timed(lambda: (idx.close(), gpu.VectorIndex(vec_ids, x2))[1].close())
        del x2
        row("vectors", n, ms, ms_pin)

if t is not None and 10000 < N:
    say("# a batch of 1024 queries, nprobe 10, k 5: medians of %d calls; scan = the scan kernel's time in the handle's profile" % REPS)
    say("# handle                                  call_ms   scan_ms")
    qs = np.ascontiguousarray(xh[rng.choice(N, 1024, replace=False)])

    def batch(idx, what):
        idx.search(qs, 5, 10)
        ts = [timed(lambda: idx.search(qs, 5, 10))[1] for _ in range(REPS)]
        idx.profile_enable(True)
        idx.search(qs, 5, 10)
        prof = idx.profile_read()
        idx.profile_enable(False)
        scan = sum(ms for nm, (_, ms) in prof.items() if nm in ("ivf_filter", "sparse_items"))
        say(f"{what:38s} {statistics.median(ts):8.3f}  {scan:8.3f}")

    at, new_cell, new_codes = ivf_payload(10000)
    idx = gpu.IVFIndex(t["coarse"], t["codebook"], t["list_off"], t["ids"], t["codes"])
    batch(idx, "fresh pin")
    idx.update_rows(t["ids"][at], coarse_id=new_cell, codes=new_codes)
    batch(idx, "after update_rows of 10 000 rows")
    idx.close()
    cell2, codes2 = cell.copy(), t["codes"].copy()
    cell2[at], codes2[at] = new_cell, new_codes
    idx = gpu.IVFIndex(*ivf_lists(t, t["ids"], cell2, codes2))
    batch(idx, "fresh pin of the updated table")
    idx.close()
out.close()
