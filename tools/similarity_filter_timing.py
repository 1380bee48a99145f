"""GPU-box helper: option similarity_filter (csrc/similarity_filter.h) against today's join on the bench's vector table (3 M x 300), one
MI355X.  Values 0 / 1 / 2 ALTERNATED on one handle, ROUNDS (3) rounds, at 100 x 3 M, 1 024 x 100 000 and 4 096 x 4 096 (A by vectors) and at
thresholds that pass about 0 / 0.01 / 0.1 / 1 / 10 % of the pairs (quantiles of a sample of the matrix).  Equal outputs are asserted before
anything is timed: the totals always, the triples where there are at most 4 M of them.  Timed: the count call (max_pairs = 0: the same
kernels but the fill, no result stream), wall clock and the kernels' sum from the handle's profile; the spread of value 0's own rounds is
recorded beside the medians.  The crossover -- the density from which value 2 no longer beats value 0 at the worse shape -- and the
SIMF_DENSE_DIV that follows from halving it are printed last.  Writes profiles/similarity_filter_timing.txt anew.  N / ROUNDS from the
environment for a smaller run."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd")]
from freddy_amd import gpu, index_build as ib   # noqa: E402

N, ROUNDS = int(os.environ.get("N", 3000000)), int(os.environ.get("ROUNDS", 3))
DENSITIES = (0.0, 1e-4, 1e-3, 1e-2, 1e-1)
out = open(os.path.join(ROOT, "profiles", "similarity_filter_timing.txt"), "w")


def say(line):
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def run(vec, mode, a, b, thr, max_pairs):
    vec.set_option("similarity_filter", mode)
    vec.profile_enable(True)
    t = time.perf_counter()
    res = vec.similarity_join(a, b, thr, max_pairs)
    wall = (time.perf_counter() - t) * 1e3
    prof = vec.profile_read()
    vec.profile_enable(False)
    return res, wall, sum(ms for _, ms in prof.values()), prof


t0 = time.time()
x = ib.make_corpus(N, seed=20260101, device=torch.device("cuda", 0))
xh = x.cpu().numpy()
del x
ids = np.arange(1, N + 1, dtype=np.int32)
vec = gpu.VectorIndex(ids, xh)
rng = np.random.default_rng(7)
say(f"# option similarity_filter 0 / 1 / 2 alternated on one handle, {N} x {xh.shape[1]}, {ROUNDS} rounds, count calls (setup {time.time() - t0:.0f} s)")
say("# shape density total | kernels ms: value 0 (min .. max of its rounds), 1, 2 | call ms: 0, 1, 2 | value 2 / value 0 (kernels) | path of value 1")
cross = {}
for na, nb in ((100, N), (1024, min(N, 100000)), (4096, min(N, 4096))):
    a = xh[rng.choice(N, na, replace=False)]
    b = ids[rng.choice(N, nb, replace=False)] if nb < N else ids
    sample = vec.similarity_matrix(a[:64], b[rng.choice(nb, min(nb, 20000), replace=False)])[0].ravel()
    for dens in DENSITIES:
        thr = np.float32(2.0) if dens == 0.0 else np.float32(np.quantile(sample, 1.0 - dens))
        ref = run(vec, 0, a, b, thr, 0)[0]
        full = ref[3] <= 4000000
        if full:
            ref = run(vec, 0, a, b, thr, ref[3])[0]
        for mode in (1, 2):
            got = run(vec, mode, a, b, thr, ref[3] if full else 0)[0]
            assert got[3] == ref[3], (na, nb, dens, mode, got[3], ref[3])
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
        kern, wall, path = {0: [], 1: [], 2: []}, {0: [], 1: [], 2: []}, ""
        for _ in range(ROUNDS):
            for mode in (0, 1, 2):
                _, w, k, prof = run(vec, mode, a, b, thr, 0)
                kern[mode].append(k)
                wall[mode].append(w)
                if mode == 1:
                    path = "filter" if "sim_matrix_kernel" not in prof else "fallback"
        k = {m: statistics.median(v) for m, v in kern.items()}
        w = {m: statistics.median(v) for m, v in wall.items()}
        ratio = k[2] / k[0]
        cross.setdefault(dens, []).append(ratio)
        say(f"{na} x {nb}  {dens:.4%}  {ref[3]} | {k[0]:.3f} ({min(kern[0]):.3f} .. {max(kern[0]):.3f})  {k[1]:.3f}  {k[2]:.3f} | "
            f"{w[0]:.3f}  {w[1]:.3f}  {w[2]:.3f} | {ratio:.3f} | {path}")
# the crossover at the worse of 100 x N and 4096 x 4096 (the issue's two shapes): the smallest measured density at which value 2 loses
losing = [d for d in DENSITIES if max(cross[d][0], cross[d][-1]) >= 1.0]
if losing:
    say(f"# value 2 stops beating value 0 at a density of {losing[0]:.4%} (the worse of the first and the last shape); halved: SIMF_DENSE_DIV = {int(round(2 / losing[0]))}")
else:
    say(f"# value 2 beats value 0 at every measured density up to {DENSITIES[-1]:.0%}: the crossover lies above it; SIMF_DENSE_DIV = {int(round(2 / DENSITIES[-1]))} halves the last density measured")
vec.close()
