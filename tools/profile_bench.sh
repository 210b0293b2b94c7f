#!/bin/bash
# GPU box: kernel-trace + the two PMC passes of the bench command (the program directly after `--`); outputs under gpurun_out/prof_<tag>_*.
# every pass is one process under its own time limit; set -e ends the script at the first pass that fails
# usage: tools/profile_bench.sh <tag>      then: python3 tools/summarize_prof.py <tag>
set -e
TAG=${1:-r03}
cd /tmp && export TMPDIR=/tmp
R=$(cd "$OLDPWD" && cd "$(dirname "$0")/.." && pwd)      # the repository this script lies in
OUT=$R/gpurun_out
mkdir -p $OUT
ARGS="--full --steps 200 --warmup 20 --no-cpu --no-cfg3"
timeout -k 10 540 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_trace -- python3 $R/bench.py $ARGS > $OUT/prof_${TAG}_trace.json 2> $OUT/prof_${TAG}_trace.log
echo "trace pass done" 
timeout -k 10 540 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof_${TAG}_fetch -- python3 $R/bench.py $ARGS > $OUT/prof_${TAG}_fetch.json 2> $OUT/prof_${TAG}_fetch.log
echo "fetch pass done"
timeout -k 10 540 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof_${TAG}_write -- python3 $R/bench.py $ARGS > $OUT/prof_${TAG}_write.json 2> $OUT/prof_${TAG}_write.log
echo "write pass done"
# L2 requests of the headline kernel (how many reads the CUs send to L2, and what L2 sees and hits): one counter per run, plain bench
LEAN="--steps 200 --warmup 20"
for CTR in TCP_TCC_READ_REQ_sum TCC_REQ_sum TCC_HIT_sum; do
    timeout -k 10 300 rocprofv3 --pmc $CTR --output-format csv -d $OUT/prof_${TAG}_$CTR -- python3 $R/bench.py $LEAN > $OUT/prof_${TAG}_$CTR.json 2> $OUT/prof_${TAG}_$CTR.log
    echo "$CTR pass done"
done
cd $R && python3 tools/summarize_prof.py $TAG --stage-only
