#!/bin/bash
# timeline of the fused V launch, dataflow tail against the barrier tail (diagnostic builds: scripts/ab_build.sh stamps "-DBTF_ACC_STAMPS"):
#   scripts/stamps_df_ab.sh [lib tags, default "stamps"]     (timelines under $STAMPS_DIR, default build/stamps)
cd "$(dirname "$0")/.."
out=${STAMPS_DIR:-build/stamps}
mkdir -p "$out"
for tag in ${@:-stamps}; do
  for df in 1 0 1 0; do
    echo "=== lib $tag dataflow=$df"
    BTF_VF_DATAFLOW=$df BTF_LIB_PATH=$PWD/functionalmf_amd/libbtf_$tag.so BTF_ACC_STAMPS_OUT=$out/st_${tag}_$df.npz timeout -k 10 300 python bench.py --full --steps 100 --no-cpu --no-c4 --lean 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['kernels_us'])"
    python scripts/acc_stamps.py $out/st_${tag}_$df.npz | grep -A14 "^v accumulation"
  done
done
