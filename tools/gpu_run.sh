#!/bin/bash
# GPU-box driver script for one session: tests, benches, one rocprofv3 kernel trace.  Everything lands in $OUT_DIR/<tag>_* (default runs/).
# usage: tools/gpu_run.sh <tag> [pytest -k expression | all | none] [bench configs...]
tag=${1:-r2a}; ksel=${2:-all}; shift; shift
root=$(pwd); out=$(realpath -m "${OUT_DIR:-runs}")
mkdir -p $out
export TMPDIR=/tmp
if [ "$ksel" != "none" ]; then
  if [ "$ksel" == "all" ]; then kflag=(); else kflag=(-k "$ksel"); fi
  python -m pytest tests -m gpu -q -x --timeout=900 "${kflag[@]}" > $out/${tag}_tests.log 2>&1
  echo "tests rc=$?" >> $out/${tag}_tests.log
  tail -5 $out/${tag}_tests.log
fi
cfgs=("$@")
if [ ${#cfgs[@]} -eq 0 ]; then cfgs=("std:" "nodefer:--no-defer" "large:--tile large" "dp1:--dp-selftest --no-cpu-baseline" "tsrn:--arch tsrn --no-cpu-baseline" "tbsrn:--arch tbsrn --no-cpu-baseline"); fi
for cfg in "${cfgs[@]}"; do
  name=${cfg%%:*}; flags=${cfg#*:}
  [ "$name" == "skip" ] && continue
  timeout 600 python bench.py --full --steps 20 --warmup 5 $flags > $out/${tag}_bench_${name}.json 2> $out/${tag}_bench_${name}.err
  echo "bench $name rc=$? $(cut -c1-200 $out/${tag}_bench_${name}.json)"
done
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $out/${tag}_prof -o p -- python $root/bench.py --steps 10 --warmup 5 --no-cpu-baseline > $out/${tag}_prof.log 2>&1
cd $root
db=$(find $out/${tag}_prof -name "*.db" | head -1)
python tools/prof_summary.py $db 15 > $out/${tag}_kernel_stats.txt 2>&1
head -12 $out/${tag}_kernel_stats.txt
