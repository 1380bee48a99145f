#!/usr/bin/env python3
"""GPU-box helper: randomised comparison of the IVFADC search on index shapes OTHER than m = 12 / S = 25 (multi.h's cell-grouped
exact scan, the generic kernels behind it) and on the filter + refine scan with the running bound, against the CPU oracle.  The draws
are tests/soak_inputs.py's (draw_shapes) and the comparison is tests/test_gpu_soak.py's (run_shapes): the suite runs the first
len(soak_inputs.SEEDS["shapes"]) seeds of this loop.
usage: python tools/soak_shapes.py [seeds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu
from oracle.oracle import Oracle
import soak_inputs as si
import test_gpu_soak as ts

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 24
oracle = Oracle()
gpu.load()
t0 = time.time()
for seed in range(seeds):
    d = si.draw_shapes(seed, oracle)
    ts.run_shapes(gpu, d)
    print(f"{d['label']} ok ({time.time() - t0:.0f} s)", flush=True)
print("soak_shapes ok")
