#!/usr/bin/env python3
"""GPU-box helper: randomised comparison of the re-ranking entry points -- search_pv, the approximate analogies, PQIndex.assign and
PQIndex.search_pv over a subset, on an IVFIndex or a PQIndex with the VectorIndex of most of the same rows -- against pv_model,
approx_analogy_model and assign_model.  The draws are tests/soak_inputs.py's (draw_rerank) and the comparison is
tests/test_gpu_soak_rerank.py's (run): the suite runs the first len(soak_inputs.SEEDS["rerank"]) seeds of this loop.
usage: python tools/soak_rerank.py [seeds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu
from oracle.oracle import Oracle
import soak_inputs as si
import test_gpu_soak_rerank as tk

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 48
oracle = Oracle()
gpu.load()
t0 = time.time()
for seed in range(seeds):
    d = si.draw_rerank(seed, oracle)
    tk.run(gpu, d)
    print(f"{d['label']} ok ({time.time() - t0:.0f} s)", flush=True)
print("soak_rerank ok")
