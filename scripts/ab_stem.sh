#!/bin/bash
# the fp32-clip stem under the values of one switch taking turns on one box (scripts/stem_clip_probe.py, 375 clips): bash scripts/ab_stem.sh ["values"] [VAR]
#   bash scripts/ab_stem.sh "0 4 8"                       without / with 4 / with 8 loader waves (TEDSPAD_STEM_LOADERS, the default)
#   bash scripts/ab_stem.sh "0 1" TEDSPAD_STEM_UNIFORM    the loader waves' per-lane task deal / one (frame, half) per wave
set -o pipefail
VAR=${2:-TEDSPAD_STEM_LOADERS}
for r in 1 2; do
  for v in ${1:-0 4 8}; do
    echo "== $VAR=$v round $r"; env $VAR=$v timeout -k 10 300 python scripts/stem_clip_probe.py 375 2>&1 | tail -6 || exit 1
  done
done
