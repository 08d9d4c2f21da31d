#!/bin/bash
# Same-box A/B of two library builds: alternating bench runs (VQ-VAE line + transformer line), ARCWELD_LIB selects
# the build.  usage: [OUT=dir] bash tools/ab_bench.sh <libA.so> <libB.so> [rounds]
# Both builds must have this tree's AW_ABI_VERSION (the host refuses any other library): an A/B across an ABI change
# needs two trees, each running its own bench.py against its own build.
set -o pipefail
A=$1; B=$2; R=${3:-2}
OUT=${OUT:-build/ab}
mkdir -p $OUT
for i in $(seq 1 $R); do
  for L in A B; do
    lib=$A; [ $L = B ] && lib=$B
    ARCWELD_LIB=$lib timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-profile > $OUT/$L$i.log 2>&1 || exit 1
    tail -1 $OUT/$L$i.log | python -c "import json,sys;d=json.loads(sys.stdin.read());print('$L', d['value'], d['lines']['transformer']['value'])"
  done
done
