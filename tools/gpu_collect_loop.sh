#!/bin/bash
# The collection loop (Learner::CollectLoop, rlgpu_envset_collect_loop) measured on one box:
#   bound    tools/collect_loop_bound.py: the per-workgroup cycle sums that bound what the loop can save
#   ab       three alternating bench pairs against the parent commit's tree built at $PARENT (A), then one pair of
#            --steps 20 --warmup 5; the last pair of the three also dumps its outputs, compared byte for byte
#   trace    one iteration under rocprofv3 --kernel-trace: the kernels of the collection phase
# Every GPU step runs under its own timeout; the first failure ends the script.
# usage: [OUT=dir] TAG=name PARENT=dir bash tools/gpu_collect_loop.sh bound ab trace   (writes under $OUT/$TAG)
O=${OUT:-bench_out}/${TAG:-collect_loop}
mkdir -p $O
line() {  # the phases of a bench line
  python -c "
import json, sys; d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); p = {k: round(v * 1e3, 1) for k, v in d['phase_s_per_iteration'].items()}
print(sys.argv[2], round(d['value']), round(d['ms_per_step'], 2), json.dumps(p), 'env_ms', d['roofline'].get('kernel_ms'), 'launch_arenas', d['roofline'].get('units_per_launch'))" "$1" "$2"
}
for what in "$@"; do
  case $what in
  bound)
    timeout -k 10 300 python -u tools/collect_loop_bound.py > $O/bound.txt 2>&1 || { tail -20 $O/bound.txt; exit 1; }
    cat $O/bound.txt ;;
  ab)
    for i in 1 2 3 4; do
      S="--steps 6 --warmup 1"; [ $i = 4 ] && S="--steps 20 --warmup 5"
      D=""; [ $i = 3 ] && D="--dump-outputs"
      timeout -k 10 400 python $PARENT/bench.py --gpus 1 $S --no-cpu-baseline ${D:+$D $O/dump_a} > $O/a$i.log 2>&1 || { tail $O/a$i.log; exit 1; }
      timeout -k 10 400 python bench.py --gpus 1 $S --no-cpu-baseline ${D:+$D $O/dump_b} > $O/b$i.log 2>&1 || { tail $O/b$i.log; exit 1; }
      for ab in a b; do echo "$ab$i $(tail -1 $O/$ab$i.log)" >> $O/ab_lines.txt; line $O/$ab$i.log "$ab$i" | tee -a $O/ab_summary.txt; done
    done
    for f in $O/dump_a/*.npy; do cmp $f $O/dump_b/$(basename $f) && echo "same $(basename $f)"; done | tee $O/dump_cmp.txt
    echo "$(grep -c '^same' $O/dump_cmp.txt) of $(ls $O/dump_a/*.npy | wc -l) dumped arrays byte-equal" | tee -a $O/ab_summary.txt
    rm -rf $O/dump_a $O/dump_b ;;
  trace)
    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/t -o run -- python3 bench.py --gpus 1 --steps 1 --warmup 1 --no-cpu-baseline > $O/t.log 2>&1 || { tail -20 $O/t.log; exit 1; }
    f=$(find $O/t -name 'run_kernel_trace.csv' | head -1)
    python tools/collect_loop_trace.py $f | tee $O/trace.txt || exit 1
    rm -rf $O/t ;;
  esac
done
