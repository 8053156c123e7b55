"""Detector every Nth frame: the two measurements of profiles/r10/detect_every.txt.

1. Kernel time of the propagation pair (csrc/maskprop.hip) at 480x640, one process under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_detect_every.py kernels
    python tools/prof_detect_every.py parse DIR

   `kernels` runs HipOps.mask_propagate 70 times with a depth map and 70 times without on a seeded blob image (a third of the pixels labelled) and a flow of +-12 px;
   `parse` prints median / min / max of the last 60 launches of each block for k_maskprop_scatter and k_maskprop_resolve, and of whatever other kernels ran between them
   (the runtime's fill kernels behind the call's two memsets).

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip (synth.convoy_scene, feed="given", device hand-over) at detect_every 1, 2 and 3, one process, ONE set of
   networks, the cadences alternating round by round so that drift of the machine falls on all three alike:

    python tools/prof_detect_every.py e2e [--steps 100] [--warmup 20] [--rounds 3]

   The parent commit is measured the same way from a CHECKOUT of the parent (its own package and library) with this file copied into its tools/: `e2e --only 1` constructs
   NetNodes without the argument and never touches the cadence."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernels():
    import numpy as np
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets
    H, W = 480, 640
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    rng = np.random.RandomState(7)
    m = np.zeros((H, W), np.int32); yy, xx = np.mgrid[0:H, 0:W]
    for i in range(9):
        cy, cx, ry, rx = rng.randint(40, H - 40), rng.randint(40, W - 40), rng.randint(30, 90), rng.randint(40, 120)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = i + 1
    f = rng.uniform(-12, 12, (H, W, 2)).astype(np.float32); d = rng.uniform(2, 40, (H, W)).astype(np.float32)
    tm, tf, td = torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()
    out = torch.empty_like(tm); st = torch.zeros(3, dtype=torch.int32, device="cuda")
    for depth in (td, None):
        for _ in range(70):
            ops.mask_propagate(tm, tf, depth, out=out, stats=st)
        torch.cuda.synchronize()
        print("labelled %.3f of the pixels; stats (sources, hit, filled) %s, depth %s" % (float((tm > 0).float().mean()), st.tolist(), depth is not None))


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(f) == 1, f
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_maskprop_scatter"))
    last = max(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_maskprop_resolve"))
    by = {}
    for r in rows[max(first - 2, 0):last + 1]:                      # (the first call's fills come just before its scatter)
        by.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for name, ns in by.items():
        if len(ns) % 140:
            print("%s: %d launches in the window (not a multiple of the 140 calls), all of them: median_ns %.0f" % (name, len(ns), statistics.median(ns))); continue
        per = len(ns) // 140
        for blk, lo in (("with_depth", 10 * per), ("without_depth", 80 * per)):
            b = ns[lo:lo + 60 * per]
            print("%s %s x%d per call: median_ns %.0f min_ns %d max_ns %d n %d" % (name, blk, per, statistics.median(b), min(b), max(b), len(b)))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, default=0, help="measure this one cadence (1: also in a checkout of the parent commit, the cadence is never touched)")
    a = ap.parse_args(argv)
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System
    from bench import write_settings                                  # the bench's settings for its clip
    W, H = 640, 480
    n_total = a.warmup + a.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5)
    from concurrent.futures import ThreadPoolExecutor
    def render(k):
        g, d, f, m = scene.frame(k)
        return synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_detect_every_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W)
    cadences = [a.only] if a.only else [1, 2, 3]
    res = {n: [] for n in cadences}
    for rnd in range(a.rounds):
        for n in cadences:
            if not (a.only == 1):
                nodes._set_detect_every(n)
            runs0 = getattr(nodes, "detector_runs", 0)
            slam = System(); slam.Init(cfg, System.RGBD)      # (one System at a time; each run tracks the clip from its first frame)
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
            res[n].append(a.steps / dt)
            print("round %d detect_every %d: %.1f frames/s over %d steps (%d detector runs in %d frames)" % (rnd, n, a.steps / dt, a.steps, getattr(nodes, "detector_runs", 0) - runs0, n_total), flush=True)
    for n in cadences:
        v = res[n]
        print("detect_every %d: frames/s %s  mean %.1f  min %.1f  max %.1f" % (n, " ".join("%.1f" % x for x in v), sum(v) / len(v), min(v), max(v)))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
