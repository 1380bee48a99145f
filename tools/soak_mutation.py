#!/usr/bin/env python3
"""GPU-box helper: randomised walks of ten steps -- append_rows, remove_rows, update_rows, update_codebook and one refused call --
on a handle of every kind, compared after every step with the CPU oracle on update_model's tables and at four steps with a fresh
pin.  The draws are tests/soak_inputs.py's (draw_mutation) and the comparison is tests/test_gpu_soak_mutation.py's (run): the suite
runs the first len(soak_inputs.SEEDS["mutation"]) seeds of this loop.
usage: python tools/soak_mutation.py [seeds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu
from oracle.oracle import Oracle
import soak_inputs as si
import test_gpu_soak_mutation as tm

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 24
oracle = Oracle()
gpu.load()
t0 = time.time()
for seed in range(seeds):
    for kind in si.MUTATION_KINDS:
        d = si.draw_mutation(kind, seed, oracle)
        tm.run(gpu, oracle, d)
        print(f"{d['label']} ok ({time.time() - t0:.0f} s)", flush=True)
print("soak_mutation ok")
