"""The detector's stem and the RPN's 1x1 heads inside the detector graph: the measurements of profiles/r13/detector_stem_rpn.txt.

    python tools/prof_detector_stem_rpn.py det [--frames 25:125] [--reps 5]
        the detector as bench.py builds it (pipeline.NetNodes defaults, ONE captured graph) replayed alone over the clip bench.py times (synth.convoy_scene(126, seed=5),
        frames 25 .. 124): the graph's replay time by device events, `reps` blocks of one replay per frame, the per-replay mean of each block and the spread inside the
        process.  VIDO_NO_STEM_FUSED=1 / VIDO_SKINNY_DEPTH=4 in the environment measure each switch in the same tree; the parent commit is measured from a checkout of it
        with this file copied in.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_detector_stem_rpn.py det --reps 1
    python tools/prof_detector_stem_rpn.py parse DIR [--copy-rate GB_PER_S]
        (a trace run of its own: never together with counters) medians over the last 100 replays of the stem's launches — the library's strided 7x7 convolution, the
        bias + ReLU pass and the max-pool behind it, or the one k_stem7x7s2_pool — and of the five k_conv1x1_skinny<1, false> launches of the RPN heads, level by level;
        the heads' 74 MB set against the copy rate the stem's k_bias_act pass reaches in the same trace (2 x 55.7 MB; where the trace has no such pass, --copy-rate takes the
        figure of the trace that has)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEM_MAP_BYTES = 64 * 400 * 544 * 4                      # the stem convolution's output at 800 x 1088
HEAD_BYTES = 74e6                                        # the five levels' 256-channel maps + the 15-channel outputs


def det(argv):
    import argparse
    import torch
    import __graft_entry__ as ge
    ge.build()
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    ap = argparse.ArgumentParser(); ap.add_argument("--frames", default="25:125"); ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    lo, hi = (int(v) for v in a.frames.split(":"))
    W, H = 640, 480
    scene = synth.convoy_scene(126, w=W, h=H, seed=5)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        frames = list(pool.map(lambda k: torch.as_tensor(synth.gray_to_bgr(scene.frame(k)[0])), range(lo, hi)))
    ctx = V.Context(width=W, height=H, max_batch=1)
    nodes = pipeline.NetNodes(ctx, H, W)
    assert nodes.g_det is not None, nodes.graph_error
    frames = [f.cuda() for f in frames]
    tag = " ".join("%s=%s" % (k, os.environ[k]) for k in ("VIDO_NO_STEM_FUSED", "VIDO_SKINNY_DEPTH") if os.environ.get(k)) or "default"
    for f in frames:                                                          # (one pass to warm up)
        nodes.g_det(f)
    t = []
    for r in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for f in frames:
            nodes.g_det(f)
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / len(frames))
    print("## detector alone, %s, frames %d .. %d" % (tag, lo, hi - 1))
    print("graph replay, ms per frame, block by block: " + " ".join("%.3f" % v for v in t) + "   min %.3f max %.3f spread %.3f" % (min(t), max(t), max(t) - min(t)))
    ctx.close()


def parse(argv):
    import argparse, csv, glob, statistics
    ap = argparse.ArgumentParser(); ap.add_argument("dir"); ap.add_argument("--copy-rate", type=float, default=None)
    a = ap.parse_args(argv)
    f = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    assert f, "no kernel trace under " + a.dir
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    # a replay of the detector graph: from one k_det_order to the next (one per replay, behind every convolution of the trunk); the last 100 replays are the timed block.
    # Behind k_det_order a replay only has its mask head, so the first strided library convolution / fused stem launch of a segment is the NEXT replay's stem.
    idx = [i for i, r in enumerate(rows) if "k_det_order" in r["Kernel_Name"]][-101:]
    per, span = {}, []

    def add(key, r):
        per.setdefault(key, []).append(us(r))
    for s, e in zip(idx[:-1], idx[1:]):
        seg = rows[s:e]
        span.append((int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3)
        names = [r["Kernel_Name"] for r in seg]
        fused = next((i for i, n in enumerate(names) if "k_stem7x7s2_pool" in n), None)
        if fused is not None:
            add("stem 1/1 k_stem7x7s2_pool", seg[fused])
        else:
            c = next((i for i, n in enumerate(names) if "stride2" in n and "miopen" in n.lower()), None)
            if c is not None:
                add("stem 1/3 " + names[c][:40], seg[c])
                b = next((i for i in range(c + 1, len(seg)) if "k_bias_act" in names[i] or "k_bias_res_act" in names[i]), None)
                p = next((i for i in range(c + 1, len(seg)) if "max_pool" in names[i]), None)
                if b is not None: add("stem 2/3 k_bias_act", seg[b])
                if p is not None: add("stem 3/3 max_pool_forward_nchw", seg[p])
        k = 0
        for r in seg:
            n = r["Kernel_Name"]
            if "k_conv1x1_skinny<1, false" in n or "k_conv1x1_skinnyILi1ELb0" in n:
                add("rpn head level %d (P%d) %s" % (k, k + 2, n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]), r); k += 1
    print("## medians over %d replays (k_det_order to the next k_det_order), us" % len(span))
    med = {}
    for key, v in sorted(per.items()):
        med[key] = statistics.median(v)
        print("%-72s median %7.1f  min %7.1f  max %7.1f  n %d" % (key[:72], med[key], min(v), max(v), len(v)))
    stem = sum(v for k, v in med.items() if k.startswith("stem")); heads = sum(v for k, v in med.items() if k.startswith("rpn head"))
    print("stem launches, summed medians: %.1f us;  rpn 1x1 heads, summed medians: %.1f us" % (stem, heads))
    rate = a.copy_rate
    if "stem 2/3 k_bias_act" in med:
        rate = 2 * STEM_MAP_BYTES / med["stem 2/3 k_bias_act"] / 1e3
        print("copy rate of the stem's k_bias_act pass (2 x %.1f MB): %.0f GB/s" % (STEM_MAP_BYTES / 1e6, rate))
    if rate and heads:
        byte_time = HEAD_BYTES / rate / 1e3
        print("rpn 1x1 heads: %.0f MB at %.0f GB/s = %.1f us; measured / byte time = %.2f" % (HEAD_BYTES / 1e6, rate, byte_time, heads / byte_time))
    print("kernels between two k_det_order: first start to last end, median %.1f us  min %.1f  max %.1f" % (statistics.median(span), min(span), max(span)))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "det"
    if mode == "det":
        det(sys.argv[2:])
    elif mode == "parse":
        parse(sys.argv[2:])
    else:
        sys.exit("usage: prof_detector_stem_rpn.py det | parse DIR")
