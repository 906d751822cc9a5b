#!/bin/bash
# Busy cycles per XCD of plain bench.py (counters only, one group per rocprofv3 run, the program after --):
#   tools/pmc_xcd.sh <out-name> [tree]   -> prof_out/<out-name>/{SQB,TAB,FETCH}/...
# tools/pmc_xcd.yaml defines SQ_BUSY_CYCLES and TA_TA_BUSY summed per XCC (select over DIMENSION_XCC);
# FETCH_SIZE is a third pass.  [tree]: another checkout whose bench.py to run (a parent build).
# PROF_OUT: the directory the passes are written under (default prof_out/ in the repository root).
# Then: python tools/parse_pmc_xcd.py prof_out/<out-name>
set -u
cd "$(dirname "$0")/.."
ROOT=$(pwd); NAME=$1; TREE=$ROOT/${2:-.}
OUT=${PROF_OUT:-$ROOT/prof_out}/$NAME; mkdir -p "$OUT"
ARGS=${PROF_ARGS:---steps 3 --warmup 1}
cd /tmp && export TMPDIR=/tmp
for pass in SQB TAB FETCH; do
    if [ $pass = FETCH ]; then
        ctrs=FETCH_SIZE; extra=""
    else
        ctrs=$(for x in 0 1 2 3 4 5 6 7; do echo -n "${pass}_XCC$x "; done); extra="-E $ROOT/tools/pmc_xcd.yaml"
    fi
    timeout -s KILL 300 rocprofv3 $extra --pmc $ctrs --output-format csv -d "$OUT/$pass" -o run \
        -- python3 -u "$TREE/bench.py" $ARGS > "$OUT/$pass.log" 2>&1 || { echo "pmc pass $pass failed"; tail -5 "$OUT/$pass.log"; exit 1; }
    echo "pmc pass $pass ok"
done
