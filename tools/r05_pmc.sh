#!/bin/bash
# usage: tools/r05_pmc.sh <tag> [bench.py arguments]  -- PMC passes (one rocprofv3 --pmc run per counter group, nothing else traced) of
# the resident step, the summary per kernel in $OUT/<tag>_pmc_summary.txt and the traffic JSON in $OUT/<tag>_traffic.json
TAG=$1; shift
R=$GRAFT_REPO_ROOT
export OUT=${OUT:-$R/results}     # (where the outputs go)
cd $R
./tools/prof_pmc.sh $TAG --combine off "$@" > /dev/null 2>&1
python3 tools/pmc_summary.py $OUT/pmc_${TAG}_insts $OUT/pmc_${TAG}_cycles $OUT/pmc_${TAG}_cache $OUT/pmc_${TAG}_fetch $OUT/pmc_${TAG}_write $OUT/pmc_${TAG}_lds $OUT/pmc_${TAG}_ta > $OUT/${TAG}_pmc_summary.txt
python3 tools/traffic_json.py $TAG "$@" > $OUT/${TAG}_traffic.json
grep "spl_layout\|spl_count_ranges" $OUT/${TAG}_pmc_summary.txt
rm -rf $OUT/pmc_${TAG}_*/
