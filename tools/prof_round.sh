#!/bin/bash
# The round's evidence in one go (run on the GPU box):  tools/prof_round.sh <tag> [bench.py arguments, e.g. --workload arabidopsis]
#   $OUT/<tag>_bench.json.log     the bench line of that command (CPU baseline and e2e legs included)
#   $OUT/<tag>_kernel_stats.csv   rocprofv3 --kernel-trace --stats of the same command (without the CPU / e2e legs)
#   $OUT/<tag>_pmc_summary.txt    PMC means per dispatch, one --pmc pass per counter group
#   $OUT/<tag>_traffic.json       HBM bytes per launch of the range kernel from the FETCH_SIZE / WRITE_SIZE passes
TAG=$1; shift
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
export OUT=${OUT:-$R/results}     # (where the outputs go)
mkdir -p $OUT /tmp/wl
cd $R
python bench.py --full --cache /tmp/wl "$@" > $OUT/${TAG}_bench.json.log 2> $OUT/${TAG}_bench.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -- python3 $R/bench.py --full --cache /tmp/wl --no-cpu-baseline --e2e off --no-other-steps "$@" > $OUT/${TAG}_prof_bench.log 2>&1
find /tmp/prof_$TAG -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/${TAG}_kernel_stats.csv
cd $R
./tools/prof_pmc.sh $TAG "$@" > /dev/null 2>&1
python3 tools/pmc_summary.py $OUT/pmc_${TAG}_insts $OUT/pmc_${TAG}_cycles $OUT/pmc_${TAG}_cache $OUT/pmc_${TAG}_fetch $OUT/pmc_${TAG}_write $OUT/pmc_${TAG}_lds $OUT/pmc_${TAG}_ta > $OUT/${TAG}_pmc_summary.txt
python3 tools/traffic_json.py $TAG "$@" > $OUT/${TAG}_traffic.json
tail -n1 $OUT/${TAG}_bench.json.log | cut -c1-600
head -8 $OUT/${TAG}_kernel_stats.csv
