#!/bin/bash
# One-box A/B of the current build under environment switches: bash tools/exp_ab_env.sh R "ENV_A" "ENV_B" [bench args]
set -o pipefail
export TMPDIR=/tmp
R=$1; A=$2; B=$3; X=${4:-}
ARGS="--steps 20 --warmup 3 --no-cpu-baseline --no-train --no-bf16-leg --no-cpu-config1 $X"
for i in $(seq 1 "$R"); do
  for E in "$A" "$B"; do
    out=$(env $E timeout -k 10 120 python bench.py --full $ARGS) || exit $?
    python3 -c "import json,sys; d=json.loads(sys.argv[1]); print(sys.argv[2], d['ms_per_step'], {k: round(v, 4) for k, v in d['stage_ms'].items()})" "$out" "$E"
  done
done
