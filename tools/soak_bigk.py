#!/usr/bin/env python3
"""GPU-box helper: randomised comparison against the CPU oracle of the paths for long lists -- ivfadc_search* / pq_search* with
512 < k <= 4096 (bigk.h: selection in passes of 1024 keys, the replay in closed form, carried lists over several probing rounds)
and the kNN-join's post verification with 1024 < k * pvf <= 8192 (join_query_kernel<16, true>) -- on small tables with many
equal distances.  The draws are tests/soak_inputs.py's (draw_bigk) and the comparison is tests/test_gpu_soak.py's (run_bigk): the
suite runs the first len(soak_inputs.SEEDS["bigk"]) seeds of this loop.
usage: python tools/soak_bigk.py [seeds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "postgres-word2vec_amd"), os.path.join(ROOT, "tests")]
from freddy_amd import gpu
from oracle.oracle import Oracle
import soak_inputs as si
import test_gpu_soak as ts

seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
oracle = Oracle()
gpu.load()
t0 = time.time()
for seed in range(seeds):
    d = si.draw_bigk(seed, oracle)
    ts.run_bigk(gpu, d)
    print(f"{d['label']} ok ({time.time() - t0:.0f} s)", flush=True)
print("soak_bigk ok")
