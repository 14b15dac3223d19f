#!/bin/bash
# Evidence run for profiles/ (on the GPU box): bench line, kernel-trace stats of the same program,
# PMC passes of one full-resolution layer.   usage: tools/round_profiles.sh <tag>   (output: ${SE3_OUT_DIR:-out}/prof_<tag>)
set -u
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
prof=${SE3_OUT_DIR:-out}/prof_$tag
mkdir -p $prof
timeout -k 10 400 python bench.py --full > $prof/bench.json 2> $prof/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $prof -o stats -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-fp32 --no-graph > $prof/stats.log 2>&1
# the same statistics for the full-resolution layer alone: per-kernel averages there are level-0 launch times
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $prof -o layer -- python3 tools/profile_layer.py --reps 10 > $prof/layer.log 2>&1
bash tools/pmc_passes.sh $tag > $prof/pmc.log 2>&1
python tools/pmc_summary.py ${SE3_OUT_DIR:-out}/pmc_$tag > $prof/pmc_summary.txt 2>&1
python tools/pmc_traffic.py ${SE3_OUT_DIR:-out}/pmc_$tag $prof/traffic.json > /dev/null 2>&1
python tools/report_errors.py > $prof/errors.txt 2>&1
tail -1 $prof/bench.json
find $prof -name "*kernel_stats*" | head
