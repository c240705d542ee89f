#!/bin/bash
# One gpurun call of round 4: smoke, the GPU test suite (full report), kernel traces / HBM traffic / SQ counters of the quoted workloads -- the
# NLMPC ones in both forms of the solve kernel -- then the bench lines (which quote the traffic and counter summaries just measured on this
# very tree: bench.py refuses a summary stamped with another digest of the kernel sources), the phase profiles and the side-by-side tables.
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=gpurun_out; mkdir -p $O
T=${1:-r04}
( timeout 300 python -c "import __graft_entry__ as g; g.smoke()" ) > $O/${T}_smoke.log 2>&1; echo "smoke rc $?"
( timeout 1800 python -m pytest tests -m gpu -q -rA --timeout 600 2>&1 | grep -v "^PASSED" ) > $O/${T}_pytest.log 2>&1; tail -3 $O/${T}_pytest.log | cut -c1-220
timeout 300 tools/profile.sh $T lmpc20_b4096 --steps 60 --warmup 10 --nlmpc-extra 0
timeout 300 tools/profile.sh $T lmpc50_b32768 --config 4 --steps 10 --warmup 2
timeout 400 tools/profile.sh $T ugv_b4096 --workload ugv --steps 3 --warmup 1
timeout 400 tools/profile.sh $T osc8_b1024 --workload osc8 --steps 3 --warmup 1
timeout 300 tools/profile.sh $T ugv_b256 --workload ugv --batch 256 --steps 5 --warmup 1
timeout 300 tools/profile.sh $T osc8_b256 --workload osc8 --batch 256 --steps 3 --warmup 1
timeout 300 tools/profile.sh $T vanderpol_b4096 --workload vanderpol --steps 50 --warmup 5
timeout 300 tools/profile.sh $T lmpchetero20_b4096 --workload lmpc-hetero --steps 30 --warmup 3
timeout 600 tools/profile_sq.sh $T lmpc20_b4096 --steps 40 --warmup 5 --nlmpc-extra 0 > $O/${T}_sq_lmpc20.log 2>&1
timeout 900 tools/profile_sq.sh $T ugv_b4096 --workload ugv --steps 2 --warmup 1 --nlmpc-extra 0 > $O/${T}_sq_ugv4096.log 2>&1
timeout 900 tools/profile_sq.sh $T osc8_b1024 --workload osc8 --steps 2 --warmup 1 --nlmpc-extra 0 > $O/${T}_sq_osc81024.log 2>&1
timeout 600 tools/profile_sq.sh $T ugv_b256 --workload ugv --batch 256 --steps 3 --warmup 1 > $O/${T}_sq_ugv256.log 2>&1
timeout 600 tools/profile_sq.sh $T osc8_b256 --workload osc8 --batch 256 --steps 2 --warmup 1 > $O/${T}_sq_osc8256.log 2>&1
timeout 600 tools/profile_sq.sh $T vanderpol_b4096 --workload vanderpol --steps 30 --warmup 3 > $O/${T}_sq_vdp.log 2>&1
cp $O/${T}_pmc_traffic_*.json $O/${T}_sq_*.json $O/${T}_kernel_trace_stats_*.txt profiles/ 2>/dev/null
( timeout 300 python bench.py --full --steps 200 --warmup 20 ) > $O/${T}_bench_lmpc20.json 2> $O/${T}_bench_lmpc20.err; cut -c1-300 $O/${T}_bench_lmpc20.json
( MPCX_FORCE_DIST=1 timeout 200 python bench.py --full --steps 200 --warmup 20 --cpu-seconds 0 --pipeline-streams 0 --nlmpc-extra 0 ) 2> $O/${T}_bench_lmpc20_rccl1.err | grep "^{" > $O/${T}_bench_lmpc20_rccl1.json; cut -c1-200 $O/${T}_bench_lmpc20_rccl1.json
( timeout 300 python bench.py --full --config 4 --steps 20 --warmup 3 --cpu-seconds 0 --pipeline-streams 0 ) > $O/${T}_bench_lmpc50.json 2> $O/${T}_bench_lmpc50.err; cut -c1-200 $O/${T}_bench_lmpc50.json
( timeout 300 python bench.py --full --workload lmpc-hetero --steps 50 --warmup 5 ) > $O/${T}_bench_lmpchetero.json 2> $O/${T}_bench_lmpchetero.err; cut -c1-200 $O/${T}_bench_lmpchetero.json
for w in vanderpol ugv osc6 osc8; do
  ( timeout 600 python bench.py --full --workload $w ) > $O/${T}_bench_$w.json 2> $O/${T}_bench_$w.err; cut -c1-200 $O/${T}_bench_$w.json
done
for wb in "ugv 256" "osc8 256"; do set -- $wb
  ( timeout 300 python bench.py --full --workload $1 --batch $2 --cpu-seconds 0 --steps 5 --warmup 1 ) > $O/${T}_bench_$1_b$2.json 2> $O/${T}_bench_$1_b$2.err; cut -c1-200 $O/${T}_bench_$1_b$2.json
done
for w in osc8 ugv osc6; do ( MPCX_NLMPC_FORM=wg MPCX_LIBRARY=$PWD/libmpc_amd/libmpcx_stats.so timeout 300 python tools/nlmpc_phases.py $w 256 ) > $O/${T}_phases_wg_$w.txt 2>&1; grep -v amdgpu.ids $O/${T}_phases_wg_$w.txt | tail -14; done
for w in osc8 ugv; do ( MPCX_NLMPC_FORM=wave MPCX_LIBRARY=$PWD/libmpc_amd/libmpcx_stats.so timeout 300 python tools/nlmpc_phases.py $w 1024 ) > $O/${T}_phases_wave_$w.txt 2>&1; grep -v amdgpu.ids $O/${T}_phases_wave_$w.txt | tail -9; done
( timeout 300 python tools/nlmpc_closed_loop.py; timeout 300 python tools/nlmpc_closed_loop.py 256 20 ) > $O/${T}_nlmpc_closed_loop.json 2>&1; tail -6 $O/${T}_nlmpc_closed_loop.json | cut -c1-300
tools/nlmpc_forms.sh > $O/${T}_nlmpc_forms.txt 2>&1
bash tools/gpu_occ.sh ugv > $O/${T}_nlmpc_occupancy.txt 2>&1
tools/nlmpc_latency.sh > $O/${T}_nlmpc_latency.txt 2>&1
tools/micro/latency > $O/${T}_micro_latency.txt 2>&1
