"""vido_dis_flow on the GPU: the measurements of profiles/r20/dis_flow.txt.

1. Kernel time of one call, per kernel, next to LiteFlowNet's graph in the same session, one process under the profiler:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o op -- python tools/prof_dis_flow.py kernels
    python tools/prof_dis_flow.py parse DIR

   `kernels` calls the device form on a convoy_scene pair as BGR (what NetNodes hands it) 5 + 30 times at 640 x 480, then the same at 1242 x 375 (a Scene3D pair), all at
   the defaults; then builds LiteFlowNet the way NetNodes does (fused HIP glue, pair batch), captures analyse_flow at 640 x 480 and replays the graph 5 + 30 times.  A
   16 x 16 call of the op stands before and after the replays as a marker.  `parse` cuts the trace at the calls' k_dis_ingest launches and prints, per size, the median
   kernel time of a call and of each of its kernels (summed over the levels), and the median kernel time of one LiteFlowNet replay (every kernel between the markers over
   the replays).  If a call does not cost clearly less kernel time than a replay, the first line says so.

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip (synth.convoy_scene, feed="given", device hand-over), one process per flow source; the caller alternates
   the processes:

    python tools/prof_dis_flow.py e2e --source net|dis [--steps 200] [--warmup 20]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, CALLS = 5, 30
SIZES = ((640, 480), (1242, 375))


def _bgr(g):
    import numpy as np
    return np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=1), 255 - g], axis=-1))


def kernels():
    import numpy as np
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets, synth
    ctx = V.Context(width=640, height=480, max_batch=1); ops = nets.HipOps(ctx)
    pairs = {}
    sc = synth.convoy_scene(4); pairs[SIZES[0]] = [torch.as_tensor(_bgr(sc.frame(k)[0]), device="cuda") for k in (1, 2)]
    sc = synth.Scene3D(w=1242, h=375, K=(721.5, 721.5, 620.5, 187.0)); pairs[SIZES[1]] = [torch.as_tensor(_bgr(sc.frame(k)[0]), device="cuda") for k in (1, 2)]
    tiny = [torch.as_tensor(_bgr(synth.make_frame(16, 16, seed=k)), device="cuda") for k in (1, 2)]
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    for (w, h) in SIZES:
        a, b = pairs[(w, h)]
        out = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
        for _ in range(WARM + CALLS):
            ops.dis_flow(a, b, out=out, stats=stats)
        torch.cuda.synchronize()
        print("%d x %d: stats (kept, flat, rejected, steps) %s, |flow| median %.2f px" % (w, h, stats.tolist(), float(out.norm(dim=-1).median())))
    ops2 = nets.HipOps(V.Context(width=640, height=480, max_batch=1))
    lfn = nets.fill_deterministic(nets.LiteFlowNet(ops2.correlation, epilogue=ops2.bias_act_, warp=ops2.backwarp, fused=ops2, pair_batch=True), 1).eval().cuda()
    a, b = pairs[SIZES[0]]
    with torch.no_grad():
        fn = lambda x, y: nets.analyse_flow(lfn, x, y)
        for _ in range(2):
            fn(a, b)
        torch.cuda.synchronize()
        g = nets.Graphed(fn, [a, b])
        for _ in range(WARM):
            g(*g.static_in)
        torch.cuda.synchronize()
        ops.dis_flow(tiny[0], tiny[1], coarsest=0); torch.cuda.synchronize()       # marker
        for _ in range(CALLS):
            g(*g.static_in)
        torch.cuda.synchronize()
        ops.dis_flow(tiny[0], tiny[1], coarsest=0); torch.cuda.synchronize()       # marker
    print("LiteFlowNet: %d replays of the captured graph at 640 x 480 between the markers" % CALLS)


def parse(d):
    import csv, glob, statistics
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    starts = [i for i, r in enumerate(rows) if name(r) == "k_dis_ingest"]
    n_dis = len(SIZES) * (WARM + CALLS)
    assert len(starts) == n_dis + 2, (len(starts), n_dis + 2)
    calls = []
    for k, i in enumerate(starts):                                        # a call: its k_dis_* launches up to the next call's ingest
        j = starts[k + 1] if k + 1 < len(starts) else len(rows)
        calls.append([r for r in rows[i:j] if name(r).startswith("k_dis_")])
    m1_end = starts[n_dis] + len(calls[n_dis]); m2 = starts[n_dis + 1]
    lfn = rows[m1_end:m2]
    lfn_us = sum(dur(r) for r in lfn) / CALLS / 1e3
    lines = []
    per_size = {}
    for s, (w, h) in enumerate(SIZES):
        mine = calls[s * (WARM + CALLS) + WARM:(s + 1) * (WARM + CALLS)]
        tot = [sum(dur(r) for r in c) / 1e3 for c in mine]
        per_size[(w, h)] = statistics.median(tot)
        lines.append("%d x %d, defaults, 3-channel input: %d launches per call (+ one 16-byte fill); kernel time per call, us: median %.1f min %.1f max %.1f over %d calls" % (
            w, h, len(mine[0]), statistics.median(tot), min(tot), max(tot), len(mine)))
        for kn in ("k_dis_ingest", "k_dis_down", "k_dis_patch", "k_dis_densify"):
            v = [sum(dur(r) for r in c if name(r) == kn) / 1e3 for c in mine]
            lines.append("    %-14s x%-2d median %8.1f us" % (kn, sum(1 for r in mine[0] if name(r) == kn), statistics.median(v)))
        lv = [[dur(r) / 1e3 for r in c if name(r) == "k_dis_patch"] for c in mine]
        lines.append("    k_dis_patch by level, coarsest first, median us: " + " ".join("%.1f" % statistics.median(x) for x in zip(*lv)))
        lv = [[dur(r) / 1e3 for r in c if name(r) == "k_dis_densify"] for c in mine]
        lines.append("    k_dis_densify by level, coarsest first, median us: " + " ".join("%.1f" % statistics.median(x) for x in zip(*lv)))
    lines.append("LiteFlowNet, captured graph at 640 x 480: %.1f kernels and %.1f us of kernel time per replay over %d replays" % (len(lfn) / CALLS, lfn_us, CALLS))
    ratio = per_size[SIZES[0]] / lfn_us
    head = ("one vido_dis_flow call at 640 x 480 costs %.3f of the kernel time of one LiteFlowNet replay (%.1f us against %.1f us)" % (ratio, per_size[SIZES[0]], lfn_us))
    if ratio > 0.5:
        head = "NOT CLEARLY LESS: " + head
    print("\n".join([head] + lines))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default="net"); ap.add_argument("--steps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System
    from bench import write_settings                                  # the bench's settings for its clip
    from concurrent.futures import ThreadPoolExecutor
    W, H = 640, 480
    n_total = a.warmup + a.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5)
    def render(k):
        g, d, f, m = scene.frame(k)
        return synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_dis_flow_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, flow_source=a.source)
    slam = System(); slam.Init(cfg, System.RGBD)
    e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    for k in range(a.warmup):
        e.push(frames[k][0], frames[k][1:])
    e.finish(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.warmup, n_total):
        e.push(frames[k][0], frames[k][1:])
    e.finish(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e.close(); slam.close()
    assert e.err is None, e.err
    print("flow_source %s: %.1f frames/s over %d steps after %d (graphs: flow %s, detector %s)" % (a.source, a.steps / dt, a.steps, a.warmup, nodes.g_flow is not None, nodes.g_det is not None), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
