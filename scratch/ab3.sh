#!/bin/bash
# A/B/C... of several builds of the library on one box: bash scratch/ab3.sh "libA libB libC" [bench args]   (alternating, 3 rounds)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
LIBS=$1; shift
T=$(mktemp -d)
cp chexpert_amd/libchexpert_hip.so /tmp/lib_orig.so
for r in 1 2 3; do
  for L in $LIBS; do
    cp $L chexpert_amd/libchexpert_hip.so
    timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-other-configs --steps 10 --warmup 3 "$@" > $T/ab.json 2> $T/ab.err || { tail -3 $T/ab.err; }
    python -c "
import json; d=json.load(open('$T/ab.json')); print('$L', d['value'], d['ms_per_step'], d['roofline']['kernel'], d['roofline']['avg_launch_ms'])"
  done
done
cp /tmp/lib_orig.so chexpert_amd/libchexpert_hip.so
