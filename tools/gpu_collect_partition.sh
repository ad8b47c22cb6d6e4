#!/bin/bash
# The collection groups on CU partitions (Learner::CollectGrouped, host/cu_partition.cpp), measured on one box:
#   probe    where masked streams place whole-SIMD workgroups (tests/test_collect_partition_gpu.py, printed)
#   env      env steps alone on 1 .. 16 plain and masked streams (tools/env_streams.py)
#   sweep    bench.py with RLGPU_BENCH_COLLECT_GROUPS = 1 2 4 8, with and without the per-launch timing events
#   trace    one iteration under rocprofv3 --kernel-trace per group count (tools/trace_overlap.py)
#   ab       three alternating bench pairs against the library $RLGPU_LIB_A (A), then one pair of --steps 20 --warmup 5
# usage: [OUT=dir] TAG=name bash tools/gpu_collect_partition.sh probe env sweep trace ab   (writes under $OUT/$TAG,
# OUT = bench_out by default)
O=${OUT:-bench_out}/${TAG:-collect_partition}
mkdir -p $O
B="--steps 3 --warmup 1 --no-cpu-baseline --no-legs"
line() {  # the phases of a bench line
  python -c "
import json, sys; d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); p = {k: round(v * 1e3, 1) for k, v in d['phase_s_per_iteration'].items()}
print(sys.argv[2], round(d['value']), round(d['ms_per_step'], 2), json.dumps(p), 'env_ms', d['roofline'].get('kernel_ms'))" "$1" "$2"
}
for what in "$@"; do
  case $what in
  probe)
    timeout -k 10 180 python -m pytest tests/test_collect_partition_gpu.py -x -q -s -k "unmasked or disjoint or nest" -p no:cacheprovider > $O/probe.txt 2>&1 || { tail -25 $O/probe.txt; exit 1; }
    grep -E "^\.?G=|passed" $O/probe.txt ;;
  env)
    timeout -k 10 240 python -u tools/env_streams.py 64 4096 both > $O/env_streams.txt 2>&1 || { tail $O/env_streams.txt; exit 1; }
    grep "^K=" $O/env_streams.txt ;;
  sweep)
    for tm in 1 0; do for g in 1 2 4 8; do
      RLGPU_BENCH_ENV_TIMING=$tm RLGPU_BENCH_COLLECT_GROUPS=$g timeout -k 10 240 python -u bench.py $B > $O/bench_${tm}_$g.json 2> $O/bench_${tm}_$g.err || { tail -20 $O/bench_${tm}_$g.err; exit 1; }
      line $O/bench_${tm}_$g.json "timing $tm groups $g" | tee -a $O/learner_sweep.txt
    done; done ;;
  trace)
    for g in 1 2 4 8; do
      RLGPU_BENCH_COLLECT_GROUPS=$g timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/t$g -o run -- python3 bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-legs > $O/t$g.log 2>&1 || { tail -20 $O/t$g.log; exit 1; }
      f=$(find $O/t$g -name 'run_kernel_trace.csv' | head -1)
      echo "== groups $g" | tee -a $O/trace_summary.txt
      python tools/trace_overlap.py $f | grep -v '^columns' | tee -a $O/trace_summary.txt || exit 1
      rm -f $f
    done ;;
  ab)
    for i in 1 2 3 4; do
      S="--steps 6 --warmup 1"; [ $i = 4 ] && S="--steps 20 --warmup 5"
      RLGPU_LIB=$RLGPU_LIB_A timeout -k 10 400 python bench.py $S --no-cpu-baseline > $O/a$i.log 2>&1 || { tail $O/a$i.log; exit 1; }
      timeout -k 10 400 python bench.py $S --no-cpu-baseline > $O/b$i.log 2>&1 || { tail $O/b$i.log; exit 1; }
      for ab in a b; do echo "$ab$i $(tail -1 $O/$ab$i.log)" >> $O/ab_lines.txt; line $O/$ab$i.log "$ab$i" | tee -a $O/ab_summary.txt; done
    done ;;
  esac
done
