#!/bin/bash
# Round-3 measurement pass on the GPU box (one call each part; outputs under $R3M_OUT, default /tmp/r3m, copied to profiles/ by hand).
#   part a: the driver's default command + rocprofv3 kernel stats of the same command at fewer steps
#   part b: the other lines quoted in DESIGN.md section 6
set -e
out=${R3M_OUT:-/tmp/r3m}
mkdir -p "$out"
export TMPDIR=/tmp
case "$1" in
a)
  python bench.py --full > $out/default.json 2> $out/default.err
  rm -rf $out/prof
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -- python3 bench.py --full --no-cpu-baseline --no-drop-in --steps 2 --warmup 1 > $out/prof_bench.json 2> $out/prof_bench.err
  cp $(ls $out/prof/*/*kernel_stats.csv | head -1) $out/r3_kernel_stats_default_bench.csv
  rm -rf $out/prof
  head -12 $out/r3_kernel_stats_default_bench.csv
  ;;
c)
  python tools/prof_pipeline.py 16 1 > $out/r3_count_loop_profile.txt 2>&1
  python tools/prof_batched.py > $out/r3_batched_loop_profile.txt 2>&1
  SWK_DIST_BACKEND=gloo python bench.py --full --gpus 2 --steps 3 --warmup 1 --windows 32 --no-cpu-baseline > $out/launcher_2ranks_gloo_one_gpu.json 2> $out/launcher.err
  tail -c 900 $out/launcher_2ranks_gloo_one_gpu.json
  python bench.py --full > $out/default.json 2> $out/default.err
  ;;
b)
  python bench.py --full --no-cpu-baseline --no-drop-in --size P3 --n 21 --windows 96 --steps 5 > $out/p3_n21.json 2>/dev/null
  python bench.py --full --no-cpu-baseline --no-drop-in --n 21 --windows 384 --steps 5 > $out/n21.json 2>/dev/null
  python bench.py --full --no-cpu-baseline --no-drop-in --no-classify --steps 5 > $out/segment.json 2>/dev/null
  python bench.py --full --no-cpu-baseline --no-drop-in --no-classify --steps 5 --norm-spec 0 --sparse-spec 0 > $out/spec_off.json 2>/dev/null
  python tools/bench_convs.py 4096 5 > $out/r3_cnn_layers.txt 2>&1
  python tools/bench_convs.py 256 20 > $out/r3_cnn_layers_batch256.txt 2>&1
  python tools/bench_framequeue.py > $out/framequeue.json 2>/dev/null
  python tools/prof_pipeline.py 16 1 > $out/r3_count_loop_profile.txt 2>&1
  python tools/prof_batched.py > $out/r3_batched_loop_profile.txt 2>&1
  SWK_DIST_BACKEND=gloo python bench.py --full --gpus 2 --steps 3 --warmup 1 --windows 32 --no-cpu-baseline > $out/launcher_2ranks_gloo_one_gpu.json 2> $out/launcher.err
  tail -c 600 $out/launcher_2ranks_gloo_one_gpu.json
  ;;
esac
