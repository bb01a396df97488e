#!/bin/bash
# Round recipes of the seam-repair flow, replayed on the CPU (tools/sim_tile_schedule.c, SIM_REPAIR): pass 0 on 256 x 64 tiles,
# bands astride rows 64 k, strips in 64-row slices, caps 6 / 4 -- which 256 x 32 tiles get flagged for pass 2 and how many
# rounds and sweeps every run takes, per recipe of the later rounds.
#   tools/sim_seam_round_recipes.sh WORKDIR > profiles/seam_rounds_sim.txt       (WORKDIR: where the fields are written)
set -e
root=$(cd "$(dirname "$0")/.." && pwd); work=${1:-/tmp/sim_seam}; mkdir -p "$work" "$root/tools/_build"
sim=$root/tools/_build/sim_tile_schedule
gcc -O2 -o "$sim" "$root/tools/sim_tile_schedule.c"
export SIM_REPAIR=6,4 SIM_REPAIR_GEOM=64,64 SIM_REPAIR_CAPS=6,4 SIM_MATTERS=1 SIM_REPAIR_SKIP=1
run() {      # field prefix, side, seeds, then VAR=value settings
  local f=$1 n=$2 s=$3; shift 3
  echo "--- $*"
  env "$@" "$sim" "$f.u8" "$n" "$f.seeds" "$s" 256 32 0 'DRU|L' | grep -E '^(pass 0|bands |strips|repair)' | sed -e 's/ (those need.*//'
}
for field in "2048 0" "2048 4" "2048 16" "2048 64" "8192 0"; do
  set -- $field
  f=$work/f$1_$2
  seeds=$(python3 "$root/tools/sim_make_field.py" $1 $2 "$f" | awk '{print $3}')
  echo "===== field $1 x $1, correlation $2 px (0: noise), $seeds seeds"
  # pass 0: the later rounds (bands and strips: full rounds)
  run $f $1 $seeds SIM_P0_RECIPE_LATER='|L'
  run $f $1 $seeds SIM_NOTE=full_rounds
  for d in U D R; do run $f $1 $seeds SIM_P0_RECIPE_LATER="$d|L"; done
  for d in U D R; do run $f $1 $seeds SIM_P0_RECIPE2="$d|L" SIM_P0_RECIPE_LATER="$d|L"; done
  if [ "$field" = "2048 0" ]; then
    for d in U D R L; do run $f $1 $seeds SIM_P0_RECIPE_LATER="|$d"; done
    SIM_REPAIR_CAPS=10,4 run $f $1 $seeds SIM_P0_RECIPE_LATER='|L' SIM_NOTE=cap_10
  fi
  # bands and strips, with pass 0 as chosen (a full round 1, then U|L)
  for d in U D; do run $f $1 $seeds SIM_P0_RECIPE2='U|L' SIM_P0_RECIPE_LATER='U|L' SIM_BAND_RECIPE_LATER="$d|L"; done
  run $f $1 $seeds SIM_P0_RECIPE2='U|L' SIM_P0_RECIPE_LATER='U|L' SIM_BAND_RECIPE_LATER='|L'
  run $f $1 $seeds SIM_P0_RECIPE2='U|L' SIM_P0_RECIPE_LATER='U|L' SIM_BAND_RECIPE_LATER='U|L' SIM_STRIP_RECIPE_LATER='U|L'
done
