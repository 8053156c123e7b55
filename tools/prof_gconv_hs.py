"""The detector's grouped 3x3 of 8 / 16 channels per group, fp32 matrix instruction (csrc/gconv.hip::k_gconv3x3_m16d) against split-fp16 (csrc/gconvhs.hip): the measurements
of profiles/r22/gconv_hs.txt.  The file runs in a checkout of the parent commit as well (copied in): what that tree does not have is left out of the tables.

    python tools/prof_gconv_hs.py kernel [--launches 200] [--blocks 3]
        the kernels alone on the two workload shapes (32 x 8 @ 200 x 272, 32 x 16 @ 100 x 136) and the one-group fixed-cost probe (1 x 8 @ 32 x 60): launches back to back,
        device events around blocks of `launches`, min / max of the blocks in us per launch.  VIDO_GCONV_HS_ITEMS=n cuts the new kernel's launches into n items.

    python tools/prof_gconv_hs.py det [--frames 25:125] [--reps 5]
        the detector as bench.py builds it (pipeline.NetNodes defaults, ONE captured graph) replayed over the clip bench.py times: `reps` blocks of one replay per frame,
        ms per replay of each block.  VIDO_GCONV_HS=0 in the environment: the parent's launches in this tree.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_gconv_hs.py trace
    python tools/prof_gconv_hs.py parse DIR
        `trace` = det --reps 1 followed by kernel --launches 50 --blocks 1; `parse` prints per-launch medians of the grouped 3x3 kernels by launch shape (workgroups)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("layer1 32x8  @ 200x272", 32, 8, 200, 272), ("layer2 32x16 @ 100x136", 32, 16, 100, 136), ("layer1 32x8  @ 272x200", 32, 8, 272, 200), ("layer2 32x16 @ 136x100", 32, 16, 136, 100),
          ("probe   1x8  @  32x60 ", 1, 8, 32, 60))      # (272 x 200 / 136 x 100: the maps as the detector graph launches them, rows x columns)


def kernel(argv, ctx=None):
    import argparse
    import torch
    import __graft_entry__ as ge
    ge.build()
    import vido_slam_amd as V
    from vido_slam_amd import nets
    import vido_slam_amd.nets.ops as O
    ap = argparse.ArgumentParser(); ap.add_argument("--launches", type=int, default=200); ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args(argv)
    own = ctx is None
    if own:
        ctx = V.Context(width=640, height=480, max_batch=1)
    ops = nets.HipOps(ctx)
    has_hs = hasattr(ops, "gconv3x3_hs_bias_act")

    def timed(fn):
        for _ in range(20):
            fn()
        t = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(a.launches):
                fn()
            e1.record(); torch.cuda.synchronize()
            t.append(1e3 * e0.elapsed_time(e1) / a.launches)
        return min(t), max(t)

    print("## grouped 3x3 kernels alone: us per launch (back to back, %d blocks of %d launches: min / max of the blocks), VIDO_GCONV_HS_ITEMS=%s"
          % (a.blocks, a.launches, os.environ.get("VIDO_GCONV_HS_ITEMS", "unset")))
    print("shape                  | fp32 (gconv3x3_bias_act) | split-fp16 (gconv3x3_hs_bias_act) | slowest new < fastest fp32")
    for name, G, cpg, H, W in SHAPES:
        g = torch.Generator().manual_seed(G + cpg)
        x = torch.relu(torch.randn(1, G * cpg, H, W, generator=g)).cuda(); w = torch.randn(G * cpg, cpg, 3, 3, generator=g) / (3 * cpg ** 0.5); b = torch.randn(G * cpg, generator=g).cuda()
        wp = O.pack_gconv3x3(w, G).cuda()
        lo, hi = timed(lambda: ops.gconv3x3_bias_act(x, wp, b, G, 0.0))
        cell, verdict = "      -       ", "-"
        if has_hs and ops.gconv3x3_hs_supported(H, W, cpg, cpg):
            wphs = O.pack_gconv3x3_hs(w, G).cuda()
            l2, h2 = timed(lambda: ops.gconv3x3_hs_bias_act(x, wphs, b, G, 0.0))
            cell, verdict = "%6.1f /%6.1f" % (l2, h2), "yes" if h2 < lo else "NO"
        print("%s | %6.1f /%6.1f          | %s                    | %s" % (name, lo, hi, cell, verdict))
    if own:
        ctx.close()


def det(argv, then=None):
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
    for f in frames[:5]:
        nodes.g_det(f)
    t = []
    for r in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for f in frames:
            nodes.g_det(f)
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / len(frames))
    print("## detector graph alone, VIDO_GCONV_HS=%s, frames %d .. %d" % (os.environ.get("VIDO_GCONV_HS", "unset"), lo, hi - 1))
    print("graph replay, ms per frame, block by block: " + " ".join("%.3f" % v for v in t) + "   min %.3f max %.3f spread %.3f" % (min(t), max(t), max(t) - min(t)))
    if then is not None:
        then(ctx)
    ctx.close()


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert f, "no kernel trace under " + d
    per = {}
    for r in csv.DictReader(open(f[0])):
        name = r["Kernel_Name"]
        if "k_gconv3x3" not in name:
            continue
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        wgs = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0)) // max(int(r.get("Workgroup_Size", 1)), 1)
        key = (short, wgs)
        per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("## grouped 3x3 launches in the trace: kernel, workgroups -> us per launch")
    for (name, wgs), v in sorted(per.items()):
        print("%-34s %5d wgs  median %6.1f  min %6.1f  max %6.1f  n %d" % (name[:34], wgs, statistics.median(v), min(v), max(v), len(v)))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel(sys.argv[2:])
    elif mode == "det":
        det(sys.argv[2:])
    elif mode == "trace":
        det(["--reps", "1"], then=lambda ctx: kernel(["--launches", "50", "--blocks", "1"], ctx))
    elif mode == "parse":
        parse(sys.argv[2])
    else:
        sys.exit("usage: prof_gconv_hs.py kernel | det | trace | parse DIR")
