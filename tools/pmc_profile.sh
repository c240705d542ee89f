#!/bin/bash
# Runs on the GPU box: memory traffic of one bench.py workload from hardware counters, every pass a rocprofv3 run of its own that collects
# counters and nothing else (no trace domain beside them; FETCH_SIZE and WRITE_SIZE do not fit one pass).  The per-kernel means land in
# $OUT/<tag>_pmc_traffic_<wl>.json (OUT: the output directory, default profile_out), stamped with the digest of the kernel sources, from where
# they are copied to profiles/.  Run from the repository root.
#   tools/pmc_profile.sh <round-tag> <workload-tag> <bench args...>       e.g.  tools/pmc_profile.sh r07 lmpc20_b4096 --steps 60 --warmup 10
set -u
TAG=$1; WL=$2; shift 2
export TMPDIR=/tmp
OUT=${OUT:-profile_out}
mkdir -p $OUT
DIRS=""
for P in FETCH_SIZE WRITE_SIZE; do
  D=/tmp/pmc_${P}_$WL; rm -rf $D
  timeout -k 5 200 rocprofv3 --pmc $P -d $D --output-format csv -- python bench.py --full "$@" --cpu-seconds 0 --pipeline-streams 0 > $OUT/${TAG}_pmc_${P}_${WL}.log 2>&1 || { echo "pass $P failed"; exit 1; }
  DIRS="$DIRS $D"
done
python tools/pmc_summary.py $DIRS > $OUT/${TAG}_pmc_traffic_${WL}.json
cat $OUT/${TAG}_pmc_traffic_${WL}.json
