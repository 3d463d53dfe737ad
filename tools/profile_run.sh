#!/bin/bash
# rocprofv3 --kernel-trace --stats of the bench command, then the PMC passes (tools/pmc_run.sh); summaries land in $PROFILE_OUT
# (default profile_out/).
# usage (GPU box, repo root): bash tools/profile_run.sh <tag>
set -e
TAG=${1:-prof}
R=${GRAFT_REPO_ROOT:-$PWD}
export PROFILE_OUT=${PROFILE_OUT:-$R/profile_out}; OUT=$PROFILE_OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -- python3 $R/bench.py --steps 3 --warmup 1 --full --no-secondary --no-cpu > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_trace.log
f=$(find $OUT/${TAG}_trace -name "*kernel_stats.csv" | head -1)
cp "$f" $OUT/${TAG}_kernel_stats.csv
rm -rf $OUT/${TAG}_trace
cd $R && bash tools/pmc_run.sh ${TAG}_pmc 262144 > $OUT/${TAG}_pmc.log 2>&1
rm -rf $OUT/${TAG}_pmc_SQ_WAVES $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE $OUT/${TAG}_pmc_SQ_INSTS_SALU $OUT/${TAG}_pmc_SQ_INSTS_VALU_MFMA_MOPS_I8
