#!/bin/bash
# one GPU session: selected tests, bench configs, one rocprofv3 kernel trace + per-step timeline, under $OUT_DIR (default runs/).  usage: tools/gpu_quick.sh <tag> "<pytest -k expr|none>" [bench cfgs "name:flags" ...]
tag=$1; ksel=$2; shift; shift
root=$(pwd); out=$(realpath -m "${OUT_DIR:-runs}")
mkdir -p $out; export TMPDIR=/tmp
if [ "$ksel" != "none" ]; then
  timeout 1500 python -m pytest tests -m gpu -q --timeout=900 -k "$ksel" 2>&1 | tail -40 > $out/${tag}_tests.log
  tail -12 $out/${tag}_tests.log
fi
for cfg in "$@"; do
  name=${cfg%%:*}; flags=${cfg#*:}
  if [ "$name" == "prof" ]; then
    cd /tmp
    timeout 240 rocprofv3 --kernel-trace --stats -d $out/${tag}_prof -o p -- python $root/bench.py --steps 10 --warmup 5 --no-cpu-baseline --sustain 0 --no-exact-fp32 $flags > $out/${tag}_prof.log 2>&1
    cd $root
    db=$(find $out/${tag}_prof -name "*.db" | head -1)
    python tools/prof_summary.py $db 15 > $out/${tag}_kernel_stats.txt 2>&1
    python tools/prof_timeline.py $db > $out/${tag}_timeline.txt 2>&1
    python tools/prof_timeline.py $db --dump --json $out/${tag}_step_kernel_table.json > $out/${tag}_timeline_dump.txt 2>&1
    rm -rf $out/${tag}_prof
    head -40 $out/${tag}_timeline.txt
    continue
  fi
  timeout 300 python bench.py --full --steps 30 --warmup 10 $flags > $out/${tag}_bench_${name}.json 2> $out/${tag}_bench_${name}.err
  echo "bench $name rc=$? $(cut -c1-400 $out/${tag}_bench_${name}.json)"
done
