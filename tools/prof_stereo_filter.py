"""vido_stereo_filter on the GPU: the measurements of profiles/r26/stereo_filter.txt.

1. Kernel time of one call, per kernel, next to vido_mask_components and vido_stereo_sgm in the same session, one process under the profiler (kernel trace only):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o op -- python tools/prof_stereo_filter.py kernels
    python tools/prof_stereo_filter.py parse DIR

   `kernels` runs vido_stereo_sgm at its defaults on a Scene3D stereo pair at 640 x 480 5 + 30 times, then the filter's device form on that q4 / status 5 + 30 times at
   the defaults with every output, 5 + 30 times with min_region = 1 (the collision-depth plane alone: one counter launch and the write launch), and then
   vido_mask_components 5 + 30 times on the int32 mask that equals the filter's valid set, connectivity 4, min_area = the filter's min_region: the same union-find over
   the same pixels with the run shortcuts this op's relation forbids (maskcc.hip's kernels are the parent commit's, untouched).  `parse` cuts the trace at each call's
   first launch and prints the median kernel time of a call and of each of its kernels (the memset in front of vido_mask_components is no kernel of ours and is left out).

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip with depth_source="stereo", one process per setting; the caller alternates the processes:

    python tools/prof_stereo_filter.py e2e --filter 0|1 [--steps 150] [--warmup 20]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, CALLS = 5, 30
W, H = 640, 480
FIRST = {"sgm": "k_sgm_zero", "filter": "k_sf_local", "plane": "k_sf_zero", "cc": "k_cc_local"}
PREFIX = {"sgm": "k_sgm_", "filter": "k_sf_", "plane": "k_sf_", "cc": "k_cc_"}


def _bgr(g):
    import numpy as np
    return np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=0), 255 - g], axis=-1))


def kernels():
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets, synth
    from vido_slam_amd.host import STEREO_FILTER_MIN_REGION
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    a, b = [torch.as_tensor(_bgr(g), device="cuda") for g in synth.Scene3D(n_frames=3).stereo_frame(1, 0.5)[:2]]
    q4 = torch.empty((H, W), dtype=torch.int32, device="cuda"); status = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    disp = torch.empty((H, W), dtype=torch.float32, device="cuda"); stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(WARM + CALLS):
        ops.stereo_sgm(a, b, out=disp, q4=q4, status=status, stats=stats)
    torch.cuda.synchronize()
    print("vido_stereo_sgm %d x %d at the defaults: stats %s" % (W, H, stats.tolist()))
    out = torch.empty_like(disp); st = torch.empty_like(status); depth = torch.empty_like(disp)
    for _ in range(WARM + CALLS):
        ops.stereo_filter(q4, status, out=out, status_out=st, depth=depth, stats=stats, bf=250.0)
    torch.cuda.synchronize()
    print("vido_stereo_filter at the defaults: stats (valid in, regions removed, pixels removed, valid out) %s" % stats.tolist())
    for _ in range(WARM + CALLS):
        ops.stereo_filter(q4, status, out=out, depth=depth, stats=stats, bf=250.0, min_region=1)
    torch.cuda.synchronize()
    mask = ((status == 0) & (q4 >= 1) & (q4 <= 65535)).to(torch.int32).contiguous()
    lab = torch.empty_like(mask); cstats = torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(WARM + CALLS):
        ops.mask_components(mask, connectivity=4, min_area=STEREO_FILTER_MIN_REGION, id_base=0, cap=127, out=lab, stats=cstats)
    torch.cuda.synchronize()
    print("vido_mask_components on the valid set, connectivity 4: stats (found, dropped for area, left out, kept) %s" % cstats.tolist())


def parse(d):
    import csv, glob, statistics
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    med = {}
    lines = []
    for what, title in (("sgm", "vido_stereo_sgm, defaults (D = 128)"), ("filter", "vido_stereo_filter, defaults, every output"),
                        ("plane", "vido_stereo_filter, min_region = 1 (the collision-depth plane alone)"), ("cc", "vido_mask_components on the valid set, connectivity 4")):
        mine = [r for r in rows if name(r).startswith(PREFIX[what])]
        starts = [i for i, r in enumerate(mine) if name(r) == FIRST[what]]
        calls = [mine[i:(starts[k + 1] if k + 1 < len(starts) else len(mine))] for k, i in enumerate(starts)]
        if what == "plane":
            calls = [c for c in calls if len(c) == 2]                        # (k_sf_zero starts only the calls without labelling)
        if what == "filter":
            calls = [c[:4] for c in calls]                                      # (the plane-only calls' launches follow the last full call in the k_sf_ stream)
        assert len(calls) == WARM + CALLS, (what, len(calls))
        calls = calls[WARM:]
        tot = [sum(dur(r) for r in c) / 1e3 for c in calls]
        med[what] = statistics.median(tot)
        lines.append("%s: %d launches per call; kernel time per call, us: median %.1f min %.1f max %.1f over %d calls" % (title, len(calls[0]), med[what], min(tot), max(tot), len(calls)))
        for kn in dict.fromkeys(name(r) for r in calls[0]):
            lines.append("    %-14s median %8.1f us" % (kn, statistics.median([sum(dur(r) for r in c if name(r) == kn) / 1e3 for c in calls])))
    head = "%d x %d, one MI355X, rocprofv3 kernel trace, one process: vido_stereo_filter %.1f us per call = %.2f x vido_mask_components (%.1f us) = %.3f of vido_stereo_sgm (%.1f us)" % (
        W, H, med["filter"], med["filter"] / med["cc"], med["cc"], med["filter"] / med["sgm"], med["sgm"])
    print("\n".join([head] + lines))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", type=int, default=0); ap.add_argument("--steps", type=int, default=150); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System
    from bench import write_settings                                  # the bench's settings for its clip
    from concurrent.futures import ThreadPoolExecutor
    n_total = a.warmup + a.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5)
    def render(k):
        g, d, f, m = scene.frame(k)
        return synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32), synth.gray_to_bgr(scene.stereo_frame(k, 0.5)[1])
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_stereo_filter_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, depth_source="stereo", stereo_filter=True if a.filter else None)
    slam = System(); slam.Init(cfg, System.RGBD)
    e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    push = lambda k: e.push(frames[k][0], frames[k][1:4], right=frames[k][4])
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
    print("depth_source stereo, stereo_filter %s: %.1f frames/s over %d steps after %d (graphs: depth %s, detector %s)" % (
        "on" if a.filter else "off", a.steps / dt, a.steps, a.warmup, nodes.g_depth is not None, nodes.g_det is not None), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
