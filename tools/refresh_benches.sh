tag=r03
out=$(realpath -m "${OUT_DIR:-runs}"); export OUT_DIR=$out; mkdir -p $out
b() { name=$1; shift; timeout 200 python bench.py --full --steps 30 --warmup 10 "$@" > $out/${tag}_bench_${name}.json 2> $out/${tag}_bench_${name}.err; echo "bench $name rc=$? $(cut -c1-200 $out/${tag}_bench_${name}.json)"; }
b std
b large --tile large --no-cpu-baseline
b tsrn --arch tsrn --no-cpu-baseline
b tpg --arch tatt_tpg
b tssim --tssim --no-cpu-baseline
b dp_selftest --dp-selftest --no-cpu-baseline
tools/gpu_quick.sh ${tag}_final none "prof:" > /dev/null 2>&1
head -3 $out/${tag}_final_timeline.txt
