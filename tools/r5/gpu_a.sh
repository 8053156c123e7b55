#!/bin/bash
# round 5, call a: parity of the new blur / pyramid kernels, front-end timings (the old-vs-new legs went with the old kernels), conv1x1 microbench after the range-check fix, the headline as the round starts
set -u
OUT=gpurun_out/r5a; mkdir -p $OUT
timeout 600 python -m pytest tests/test_orb_gpu.py tests/test_system_gpu.py tests/test_track_gpu.py -m gpu -q -x 2>&1 | tail -5 | tee $OUT/pytest_orb.txt
timeout 120 python tools/prof_frontend_batch.py 2>&1 | grep "pyramid_ms" | tee -a $OUT/frontend.txt
timeout 300 python tools/prof_conv1x1.py 2>&1 | grep " -> " | cut -c1-250 | tee $OUT/conv1x1.txt
timeout 900 python bench.py --steps 60 --warmup 5 --no-extra --cpu-baseline 0 > $OUT/bench_60.json 2> $OUT/bench_60.err; echo "bench rc $?"; cut -c1-400 $OUT/bench_60.json
