#!/bin/bash
# Kernel-trace stats of one bench run per variant build
# (haskoin-node_amd/lib/<variant>/libhkv.so), for per-kernel A/B durations.
# Outputs go under $OUT (default: prof_out/).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT=${OUT:-prof_out}
mkdir -p "$OUT"
rc=0
for v in ${VARIANTS}; do
  HKV_LIB=haskoin-node_amd/lib/$v/libhkv.so timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$v" -o run \
    -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > "$OUT/prof_$v.log" 2>&1 || { rc=$?; echo "variant $v failed rc=$rc"; break; }
  echo "$v done"
done
exit $rc
