"""vido_stereo_sgm on the GPU: the measurements of profiles/r25/stereo_sgm.txt.

1. Kernel time of one call, per kernel, next to MonoDepth2's graph in the same session, one process under the profiler:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o op -- python tools/prof_stereo_sgm.py kernels
    python tools/prof_stereo_sgm.py parse DIR

   `kernels` calls the device form on a Scene3D stereo pair as BGR (what NetNodes hands it) 5 + 30 times at 640 x 480, then the same at 1242 x 375, both at D = 128 and
   the other defaults; then builds MonoDepth2 the way NetNodes does (frozen batch norms folded, fused HIP epilogues), captures analyse_depth at 640 x 480 and replays the
   graph 5 + 30 times.  A 16 x 16 call of the op stands before and after the replays as a marker.  `parse` cuts the trace at the calls' k_sgm_zero launches and prints,
   per size, the median kernel time of a call and of each of its kernels, the bytes each kernel moves on the S volume (u16 [h][w][D]) beside the eight-pass
   read-modify-write model (one store and seven read-add-store passes: 15 transits of S), and the median kernel time of one MonoDepth2 replay.

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip (synth.convoy_scene, feed="given", device hand-over), one process per depth source; the caller alternates
   the processes:

    python tools/prof_stereo_sgm.py e2e --depth net|stereo [--steps 200] [--warmup 20]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, CALLS = 5, 30
SIZES = ((640, 480), (1242, 375))
D = 128
KERNELS = ("k_sgm_zero", "k_sgm_ingest", "k_sgm_census", "k_sgm_path", "k_sgm_select")
# transits of the S volume per kernel: the zero fill writes it, the path launch adds every cell eight times (an atomic add is a read and a write at the L2), the
# selection reads it once
S_TRANSITS = {"k_sgm_zero": 1, "k_sgm_ingest": 0, "k_sgm_census": 0, "k_sgm_path": 16, "k_sgm_select": 1}
MODEL_TRANSITS = 15


def _bgr(g):
    import numpy as np
    return np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=0), 255 - g], axis=-1))


def kernels():
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets, synth
    ctx = V.Context(width=640, height=480, max_batch=1); ops = nets.HipOps(ctx)
    pairs = {}
    sc = synth.Scene3D(n_frames=3); pairs[SIZES[0]] = [torch.as_tensor(_bgr(g), device="cuda") for g in sc.stereo_frame(1, 0.5)[:2]]
    sc = synth.Scene3D(n_frames=3, w=1242, h=375, K=(721.5, 721.5, 620.5, 187.0)); pairs[SIZES[1]] = [torch.as_tensor(_bgr(g), device="cuda") for g in sc.stereo_frame(1, 0.3)[:2]]
    tiny = [torch.as_tensor(_bgr(synth.make_frame(16, 16, seed=k)), device="cuda") for k in (1, 2)]
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    for (w, h) in SIZES:
        a, b = pairs[(w, h)]
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        for _ in range(WARM + CALLS):
            ops.stereo_sgm(a, b, out=out, stats=stats, max_disp=D)
        torch.cuda.synchronize()
        print("%d x %d x %d: stats (valid, not unique, left-right, zero) %s, median valid disparity %.2f px" % (w, h, D, stats.tolist(), float(out[out > 0].median())))
    net = nets.fill_deterministic(nets.MonoDepth2(), 2).eval().cuda()
    nets.fold_batchnorm(net, ops)
    a = pairs[SIZES[0]][0]
    with torch.no_grad():
        fn = lambda x: nets.analyse_depth(net, x, feed=(192, 640), ops=ops).to(torch.float32)
        for _ in range(2):
            fn(a)
        torch.cuda.synchronize()
        g = nets.Graphed(fn, [a])
        for _ in range(WARM):
            g(*g.static_in)
        torch.cuda.synchronize()
        ops.stereo_sgm(tiny[0], tiny[1], max_disp=16); torch.cuda.synchronize()       # marker
        for _ in range(CALLS):
            g(*g.static_in)
        torch.cuda.synchronize()
        ops.stereo_sgm(tiny[0], tiny[1], max_disp=16); torch.cuda.synchronize()       # marker
    print("MonoDepth2: %d replays of the captured graph at 640 x 480 between the markers" % CALLS)


def parse(d):
    import csv, glob, statistics
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    starts = [i for i, r in enumerate(rows) if name(r) == "k_sgm_zero"]
    n_op = len(SIZES) * (WARM + CALLS)
    assert len(starts) == n_op + 2, (len(starts), n_op + 2)
    calls = []
    for k, i in enumerate(starts):                                        # a call: its k_sgm_* launches up to the next call's zero fill
        j = starts[k + 1] if k + 1 < len(starts) else len(rows)
        calls.append([r for r in rows[i:j] if name(r).startswith("k_sgm_")])
    m1_end = starts[n_op] + len(calls[n_op]); m2 = starts[n_op + 1]
    net = rows[m1_end:m2]
    net_us = sum(dur(r) for r in net) / CALLS / 1e3
    lines = []
    per_size = {}
    for s, (w, h) in enumerate(SIZES):
        mine = calls[s * (WARM + CALLS) + WARM:(s + 1) * (WARM + CALLS)]
        tot = [sum(dur(r) for r in c) / 1e3 for c in mine]
        wall = [(int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])) / 1e3 for c in mine]
        per_size[(w, h)] = statistics.median(tot)
        s_mb = w * h * D * 2 / 1e6
        lines.append("%d x %d x %d, defaults, 3-channel input: %d launches per call; kernel time per call, us: median %.1f min %.1f max %.1f over %d calls; first launch to last "
                     "end, us: median %.1f" % (w, h, D, len(mine[0]), statistics.median(tot), min(tot), max(tot), len(mine), statistics.median(wall)))
        lines.append("    S volume %.1f MB; the eight-pass read-modify-write model moves %d transits = %.0f MB; this form moves %d = %.0f MB (zero fill 1, eight atomic adds of "
                     "every cell at the L2 16, selection 1)" % (s_mb, MODEL_TRANSITS, MODEL_TRANSITS * s_mb, sum(S_TRANSITS.values()), sum(S_TRANSITS.values()) * s_mb))
        for kn in KERNELS:
            v = statistics.median([sum(dur(r) for r in c if name(r) == kn) / 1e3 for c in mine])
            mb = S_TRANSITS[kn] * s_mb
            lines.append("    %-14s median %8.1f us   S bytes %7.0f MB%s" % (kn, v, mb, "   (%.2f TB/s)" % (mb / v) if mb else ""))
    lines.append("MonoDepth2, captured graph at 640 x 480: %.1f kernels and %.1f us of kernel time per replay over %d replays" % (len(net) / CALLS, net_us, CALLS))
    head = "one vido_stereo_sgm call at 640 x 480 x %d costs %.3f of the kernel time of one MonoDepth2 replay (%.1f us against %.1f us)" % (
        D, per_size[SIZES[0]] / net_us, per_size[SIZES[0]], net_us)
    print("\n".join([head] + lines))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", default="net"); ap.add_argument("--steps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System
    from bench import write_settings                                  # the bench's settings for its clip
    from concurrent.futures import ThreadPoolExecutor
    W, H = 640, 480
    n_total = a.warmup + a.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5)
    stereo = a.depth == "stereo"
    def render(k):
        g, d, f, m = scene.frame(k)
        r = synth.gray_to_bgr(scene.stereo_frame(k, 0.5)[1]) if stereo else None
        return synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32), r
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_stereo_sgm_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, depth_source=a.depth)
    slam = System(); slam.Init(cfg, System.RGBD)
    e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    push = (lambda k: e.push(frames[k][0], frames[k][1:4], right=frames[k][4])) if stereo else (lambda k: e.push(frames[k][0], frames[k][1:4]))
    for k in range(a.warmup):
        push(k)
    e.finish(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.warmup, n_total):
        push(k)
    e.finish(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e.close(); slam.close()
    assert e.err is None, e.err
    print("depth_source %s: %.1f frames/s over %d steps after %d (graphs: depth %s, detector %s)" % (a.depth, a.steps / dt, a.steps, a.warmup, nodes.g_depth is not None, nodes.g_det is not None), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
