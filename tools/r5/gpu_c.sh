#!/bin/bash
# round 5, call c: the conv1x1 parity tests (the legs that forced the 128 x 112 tile form went with that form)
set -u
OUT=gpurun_out/r5c; mkdir -p $OUT
timeout 900 python -m pytest tests/test_maskrcnn_gpu.py -m gpu -q -x -k "conv1x1 or bottleneck" 2>&1 | tail -5 | tee $OUT/pytest_c1.txt
