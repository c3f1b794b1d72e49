#!/bin/bash
# usage: prof.sh <tag> [stats|sq|all] ; collects the rocprofv3 evidence of one build on the GPU box (default: all four runs;
# "stats": the kernel trace alone, "sq": the SQ_* counter pass alone, "stats+sq": those two).  MI355X_H264_LIB names another
# build of the library (media_amd/csrc/Makefile target `ab`).  Every run has a time limit of its own and a failed run ends
# the script: nothing more is started on a GPU that has just faulted or hung.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/gpurun_out/prof_$1
W=${2:-all}
T=${PROF_TIMEOUT:-240}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --full --no-cpu-baseline --no-plugin"
run() { echo "prof.sh: $1" && timeout -k 10 $T rocprofv3 "${@:3}" --output-format csv -d $O/$1 -- $B $2 > $O/$1.log 2>&1; }
case $W in all|stats|stats+sq) run stats "--steps 3 --warmup 1" --kernel-trace --stats || exit $?;; esac
case $W in all) run pmc_fetch "--steps 1 --warmup 1" --pmc FETCH_SIZE || exit $?
                run pmc_write "--steps 1 --warmup 1" --pmc WRITE_SIZE || exit $?;; esac
case $W in all|sq|stats+sq) run pmc_sq "--steps 1 --warmup 1" --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES || exit $?;; esac
[ -f $O/stats.log ] && tail -1 $O/stats.log | cut -c1-300
find $O -name "*.csv" | head -20
