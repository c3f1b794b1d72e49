#!/bin/bash
# usage: prof.sh <tag> ; collects the rocprofv3 evidence of one round on the GPU box
set -o pipefail
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/prof_$1
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-plugin > $O/stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-plugin > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-plugin > $O/pmc_write.log 2>&1
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES --output-format csv -d $O/pmc_sq -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-plugin > $O/pmc_sq.log 2>&1
tail -1 $O/stats.log | cut -c1-300
find $O -name "*.csv" | head -20
