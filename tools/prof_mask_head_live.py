"""The static mask head on the live slots only: the measurements of profiles/r12/mask_head_live.txt.

    python tools/prof_mask_head_live.py det [--frames 25:125] [--reps 5]
        the detector as bench.py builds it (pipeline.NetNodes defaults: calibrated scores, confidence 0.8, ONE captured graph) replayed over the clip bench.py times
        (synth.convoy_scene(126, seed=5); the default run's timed frames are 25 .. 124): per frame the live count and n_det — the two words NetNodes.last_counts hands the
        hand-over ring's `counts` —, then the graph's replay time by device events: `reps` blocks of one replay per frame, the per-replay mean of each block.
        VIDO_MASK_HEAD_ALL=1 in the environment measures the full mask head in the same tree; the parent commit is measured from a checkout of it with this file copied in.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_mask_head_live.py det --reps 1
    python tools/prof_mask_head_live.py parse DIR
        per-kernel medians of the mask head's launches inside the detector graph (the last block's replays), and the graph's span from the first to the last kernel of a replay.

    python tools/prof_mask_head_live.py forms
        the mask head's 3x3 layer (256 -> 256 on 14 x 14) at live counts 1, 2, 5, 10, 17, 25, 50, 100: every candidate form forced on a batch of exactly that many
        images (vido_conv3x3_h_bias_act_form: <4,1> is the coarse form the host picks for 100 images), and the counted launch on a batch of 100 with the form its rule
        picks (vido_conv3x3_h_live_form): the table of profiles/r14/mask_head_forms.txt.

    VIDO_MASK_HEAD_COARSE=1 in the environment (any mode): the counted launches of the mask head keep the parent's launch shapes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASK_HEAD = ("k_roi_align_nhwc", "k_conv3x3_h", "k_conv3x3_h_live", "k_conv1x1_b3<3", "k_conv1x1_b3ILi3", "k_mask_logit_select", "k_paste_label", "k_det_order")


def det(argv):
    import argparse
    import numpy as np
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
    tag = "full mask head (VIDO_MASK_HEAD_ALL=1)" if os.environ.get("VIDO_MASK_HEAD_ALL") else "default"
    live, ndet = [], []
    for f in frames:
        _, _, n_lab, n_det = nodes.g_det(f)
        live.append(int(n_lab)); ndet.append(int(n_det))
    print("## detector alone, %s, frames %d .. %d" % (tag, lo, hi - 1))
    print("live  per frame:", " ".join(str(v) for v in live))
    print("n_det per frame:", " ".join(str(v) for v in ndet))
    print("live: mean %.2f min %d max %d;  n_det: mean %.1f min %d max %d" % (np.mean(live), min(live), max(live), np.mean(ndet), min(ndet), max(ndet)))
    t = []
    for r in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for f in frames:
            nodes.g_det(f)
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / len(frames))
    print("graph replay, ms per frame, block by block: " + " ".join("%.3f" % v for v in t) + "   min %.3f max %.3f" % (min(t), max(t)))
    ctx.close()


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert f, "no kernel trace under " + d
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    # a replay of the detector graph: from one k_det_order to the next (one per replay); the last 100 replays are the timed block
    idx = [i for i, r in enumerate(rows) if "k_det_order" in r["Kernel_Name"]]
    idx = idx[-101:]
    per, span = {}, []
    for a, b in zip(idx[:-1], idx[1:]):
        seg = rows[a:b]
        span.append((int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3)
        seen = {}
        for r in seg:
            name = r["Kernel_Name"]
            if any(m in name for m in MASK_HEAD):
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                k = seen.get(short, 0); seen[short] = k + 1
                per.setdefault((short, k), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("## kernels of one replay (k_det_order to the next k_det_order), medians over %d replays, us" % len(span))
    for (name, k), v in sorted(per.items()):
        print("%-46s #%d  median %7.1f  min %7.1f  max %7.1f  n %d" % (name[:46], k, statistics.median(v), min(v), max(v), len(v)))
    print("kernels between two k_det_order: first start to last end, median %.1f us  min %.1f  max %.1f" % (statistics.median(span), min(span), max(span)))


def forms():
    import ctypes as C
    import torch
    import __graft_entry__ as ge
    ge.build()
    import vido_slam_amd as V
    from vido_slam_amd import nets
    from vido_slam_amd.nets.ops import pack_conv3x3_h
    ctx = V.Context(width=640, height=480, max_batch=1); ops = nets.HipOps(ctx); lib = ctx.lib
    g = torch.Generator().manual_seed(1)
    w = torch.randn(256, 256, 3, 3, generator=g) / 48; b = torch.randn(256, generator=g).cuda(); wp = pack_conv3x3_h(w).cuda()
    x = torch.randn(100, 256, 14, 14, generator=g).cuda()
    y = torch.empty(100, 256, 14, 14, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def timed(fn, n=200, blocks=3):
        for _ in range(20):
            fn()
        t = []
        for _ in range(blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1) / n)
        return min(t), max(t)

    def forced(live, rpw, cg):
        ops._adopt_stream()
        ctx._check(lib.vido_conv3x3_h_bias_act_form(ctx.h, P(x), P(wp), P(b), P(y), live, 256, 256, 14, 14, C.c_float(0.0), rpw, cg))
    CAND = ((4, 1), (2, 2), (2, 1), (1, 2))
    print("## conv3x3_h 256 -> 256 at 14 x 14: us per launch (back to back, 3 blocks of 200 launches: min / max of the blocks), VIDO_MASK_HEAD_COARSE=%s" % os.environ.get("VIDO_MASK_HEAD_COARSE", "unset"))
    print("## form <rpw, cg> forced on a batch of exactly `live` images (the workgroups a device-side choice of that form runs; <4,1>: the coarse form of 100 images) | the counted launch on batch 100")
    print("live | " + " | ".join("<%d,%d> %3d ch x %2d rows" % (r, c, 32 * r * c, 16 // c) for r, c in CAND) + " | counted launch: time, form the rule picks")
    for live in (1, 2, 5, 10, 17, 25, 50, 100):
        cells = []
        for r, c in CAND:
            lo, hi = timed(lambda: forced(live, r, c))
            cells.append("%6.1f /%6.1f" % (lo, hi))
        word = torch.tensor([live], dtype=torch.int32, device="cuda")
        lo, hi = timed(lambda: ops.conv3x3_h_bias_act(x, wp, b, 256, 0.0, word))
        fine, ch, br = ops.conv3x3_h_live_form(100, 256, 14, 14, live)
        print("%4d | " % live + " | ".join(cells) + " | %6.1f /%6.1f  %s %d ch x %d rows" % (lo, hi, "fine" if fine else "coarse", ch, br))
    ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "det"
    if mode == "det":
        det(sys.argv[2:])
    elif mode == "parse":
        parse(sys.argv[2])
    elif mode == "forms":
        forms()
    else:
        sys.exit("usage: prof_mask_head_live.py det | parse DIR | forms")
