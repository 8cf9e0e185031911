#!/bin/bash
# One box, the REAL step (edges + match back to back, as bench.py runs it), one setting after the other, twice over.
# (A timing loop of match launches alone is NOT a stand-in for it: the match launch that follows the edge kernel finds
# its workgroups in other slots than one that follows itself, and settings that depend on the slots rank differently.)
# The settings file holds one setting per line, short option names as tools/_options.py takes them
# ("SM_TILE_H=8 SM_DUO=1"; a blank line = the plan's own choice).
#   bash tools/sustained_ab.sh <cfg> <settings file>
if [ $# -lt 2 ]; then echo "usage: $0 <cfg> <settings file>" >&2; exit 2; fi
CFG=$1
SETTINGS=$2
{ for rep in 1 2; do
  while IFS= read -r s; do
    echo "== rep $rep: ${s:-shipped}"
    env $s timeout -k 10 100 python3 tools/sustained.py $CFG 2 ${STEPS:-10000} 2>&1 | grep "^t ="
  done < "$SETTINGS"
done; } > gpurun_out/sustained_ab.txt 2>&1
cat gpurun_out/sustained_ab.txt
