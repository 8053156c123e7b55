"""vido_dis_flow_pair on the GPU: the measurements of profiles/r21/dis_flow_pair.txt, by tools/prof_dis_flow.py's method.

1. Kernel time of one pair call beside two single calls, one process per form under the profiler, the caller alternating the processes:

    rocprofv3 --kernel-trace --output-format csv -d DIR_P -o op -- python tools/prof_dis_flow_pair.py kernels pair
    rocprofv3 --kernel-trace --output-format csv -d DIR_S -o op -- python tools/prof_dis_flow_pair.py kernels single
    python tools/prof_dis_flow_pair.py parse pair DIR_P
    python tools/prof_dis_flow_pair.py parse single DIR_S

   `kernels pair` calls HipOps.dis_flow_pair on a convoy_scene pair as BGR (what NetNodes hands it) 5 + 30 times at 640 x 480, then the same at 1242 x 375 (a Scene3D pair), at
   the defaults; `kernels single` calls HipOps.dis_flow(a, b) and HipOps.dis_flow(b, a) in turn, 5 + 30 times each pair of calls.  `parse` cuts the trace at the
   k_dis_ingest launches and prints, per size, the median kernel time of a call (`single`: of two consecutive calls, what the pair call replaces) and of each of its
   kernels, and the patch and densify launches by level.  The yardstick: a pair call under twice a single call.

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip with the op as flow source, the check off and on, one process each, the caller alternating:

    python tools/prof_dis_flow_pair.py e2e --consistency off|on [--steps 200] [--warmup 20]

   feed="given": the frames tracked are the rendered maps in both runs, so the figures compare the cost of producing the flow."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from prof_dis_flow import WARM, CALLS, SIZES, _bgr    # noqa: E402

KERNELS = ("k_dis_ingest", "k_dis_down", "k_dis_patch", "k_dis_densify", "k_flow_check")


def kernels(form):
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets, synth
    ctx = V.Context(width=640, height=480, max_batch=1); ops = nets.HipOps(ctx)
    pairs = {}
    sc = synth.convoy_scene(4); pairs[SIZES[0]] = [torch.as_tensor(_bgr(sc.frame(k)[0]), device="cuda") for k in (1, 2)]
    sc = synth.Scene3D(w=1242, h=375, K=(721.5, 721.5, 620.5, 187.0)); pairs[SIZES[1]] = [torch.as_tensor(_bgr(sc.frame(k)[0]), device="cuda") for k in (1, 2)]
    stats = torch.zeros(12, dtype=torch.int32, device="cuda")
    for (w, h) in SIZES:
        a, b = pairs[(w, h)]
        out = torch.empty((h, w, 2), dtype=torch.float32, device="cuda"); status = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        for _ in range(WARM + CALLS):
            if form == "pair":
                ops.dis_flow_pair(a, b, out=out, status=status, stats=stats)
            else:
                ops.dis_flow(a, b, out=out, stats=stats[0:4]); ops.dis_flow(b, a, out=out, stats=stats[4:8])
        torch.cuda.synchronize()
        print("%s, %d x %d: stats %s" % (form, w, h, stats.tolist()) + (", share of pixels marked %.3f" % float(torch.isnan(out[..., 0]).float().mean()) if form == "pair" else ""))


def parse(form, d):
    import csv, glob, statistics
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    starts = [i for i, r in enumerate(rows) if name(r) == "k_dis_ingest"]
    per = 1 if form == "pair" else 2                                      # ingest launches per measured unit
    assert len(starts) == len(SIZES) * (WARM + CALLS) * per, (len(starts), len(SIZES) * (WARM + CALLS) * per)
    units = []
    for k in range(0, len(starts), per):                                  # a unit: the launches from its first ingest up to the next unit's
        j = starts[k + per] if k + per < len(starts) else len(rows)
        units.append([r for r in rows[starts[k]:j] if name(r) in KERNELS])
    for s, (w, h) in enumerate(SIZES):
        mine = units[s * (WARM + CALLS) + WARM:(s + 1) * (WARM + CALLS)]
        tot = [sum(dur(r) for r in c) / 1e3 for c in mine]
        print("%s, %d x %d, defaults, 3-channel input: %d launches per %s; kernel time, us: median %.1f min %.1f max %.1f over %d" % (
            form, w, h, len(mine[0]), "pair call" if form == "pair" else "two single calls", statistics.median(tot), min(tot), max(tot), len(mine)))
        for kn in KERNELS:
            n = sum(1 for r in mine[0] if name(r) == kn)
            if n:
                print("    %-14s x%-2d median %8.1f us" % (kn, n, statistics.median([sum(dur(r) for r in c if name(r) == kn) / 1e3 for c in mine])))
        for kn in ("k_dis_patch", "k_dis_densify"):
            lv = [[dur(r) / 1e3 for r in c if name(r) == kn] for c in mine]
            print("    %s by launch, coarsest first, median us: " % kn + " ".join("%.1f" % statistics.median(x) for x in zip(*lv)))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--consistency", default="off", choices=("off", "on")); ap.add_argument("--steps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
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
    tmp = tempfile.mkdtemp(prefix="vido_dis_flow_pair_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, flow_source="dis", dis_consistency=True if a.consistency == "on" else None)
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
    print("flow_source dis, dis_consistency %s: %.1f frames/s over %d steps after %d (graphs: flow %s, detector %s)" % (
        a.consistency, a.steps / dt, a.steps, a.warmup, nodes.g_flow is not None, nodes.g_det is not None), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "kernels" and sys.argv[2] in ("pair", "single"):
        kernels(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "parse" and sys.argv[2] in ("pair", "single"):
        parse(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
