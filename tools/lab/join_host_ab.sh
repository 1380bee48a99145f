#!/bin/bash
# GPU-box helper: freddy_gpu_knn_join from pageable floats (`bench.py --config join`: 5000 / 1024 / 64 queries x 100 000 targets, a new
# target array every call) on the library in the tree against postgres-word2vec_amd/libfreddy_gpu_base.so (a build of the parent
# commit), alternating in ONE call as tools/lab/ab.sh does.  Appends its lines to profiles/join_ids_timing.txt.
# usage: tools/lab/join_host_ab.sh [rounds] [steps]
N=${1:-3}; STEPS=${2:-200}
OUT=profiles/join_ids_timing.txt
echo "# freddy_gpu_knn_join (the float entry point) on this build and on a build of the parent commit, alternated in one session; bench.py --config join, $STEPS steps, mean ms per step" | tee -a $OUT
for Q in 5000 1024 64; do
  for r in $(seq $N); do
    for v in new base; do
      if [ $v = base ]; then export FREDDY_GPU_SO=$PWD/postgres-word2vec_amd/libfreddy_gpu_base.so; else unset FREDDY_GPU_SO; fi
      timeout -k 10 170 python bench.py --config join --gpus 1 --Q $Q --steps $STEPS --warmup 5 2>/dev/null | tail -1 > /tmp/join_ab.json || exit 1
      python - "$v" "$Q" "$r" <<'P' | tee -a $OUT
import json, sys
o = json.load(open("/tmp/join_ab.json"))
print(f"#   Q = {int(sys.argv[2]):5d}  round {sys.argv[3]}  {sys.argv[1]:5s}  {o['ms_per_step']:.4f} ms per step  ({o['value'] / 1e6:.3f} M queries/s)")
P
    done
  done
done
