#!/bin/bash
# headline A/B (60 steps each)
OUT=${OUT:-bench_ab}; mkdir -p $OUT
run() { tag=$1; shift; env "$@" timeout 400 python bench.py --full --steps 60 --no-extra --cpu-baseline 0 > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err; python - $tag $OUT <<'PY'
import json, sys
d = json.loads(open("%s/bench_%s.json" % (sys.argv[2], sys.argv[1])).read().strip().splitlines()[-1])
s = d["stage_ms"]
print(sys.argv[1], d["value"], "ms/step", d["ms_per_step"], "det", s["maskrcnn_x101_fpn_ms"], "lfn", s["liteflownet_ms"], "trk", s["tracker_thread_ms"], "lba", s["local_ba_ms"], "wait_nets", s["tracker_wait_for_nets_ms"])
PY
}
run gconv_b3 A=1
run gconv_f32 VIDO_NO_GCONV_B3=1
run gconv_b3_2 A=1
run gconv_f32_2 VIDO_NO_GCONV_B3=1
