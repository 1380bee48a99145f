#!/usr/bin/env python3
"""GPU-box helper: randomised comparison of the exact entry points -- search, search over a subset, the exact join, exact_assign
and the three analogy methods, 6 - 8 calls in a random order on one VectorIndex per seed -- against the CPU oracle and the numpy
models.  The draws are tests/soak_inputs.py's (draw_exact) and the comparison is tests/test_gpu_soak_exact.py's (run): the suite
runs the first len(soak_inputs.SEEDS["exact"]) seeds of this loop.
usage: python tools/soak_exact.py [seeds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu
from oracle.oracle import Oracle
import soak_inputs as si
import test_gpu_soak_exact as te

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 48
oracle = Oracle()
gpu.load()
t0 = time.time()
for seed in range(seeds):
    d = si.draw_exact(seed, oracle)
    te.run(gpu, d)
    print(f"{d['label']} ok ({time.time() - t0:.0f} s)", flush=True)
print("soak_exact ok")
