"""vido_rectify on the GPU: the measurements of profiles/r27/stereo_rectify.txt.

1. Kernel time of one call next to vido_stereo_sgm in the same session, one process under the profiler (kernel trace only):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o op -- python tools/prof_stereo_rectify.py kernels
    python tools/prof_stereo_rectify.py parse DIR

   `kernels` rectifies a raw 640 x 480 x 3 Scene3D pair of the rig (K_raw = (500, 500, 319.5, 239.5), P = (470, 470, 319.5, 239.5), the KAIST coefficients, about
   1 degree per camera) 5 + 30 times in one launch for both cameras, 5 + 30 times the left camera alone, 5 + 30 times a grey pair (1 channel), and then runs
   vido_stereo_sgm at max_disp = 64, p2 = 100 on the rectified pair 5 + 30 times.  `parse` prints the median kernel time of each group.

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip with depth_source="stereo", with raw pairs and NetNodes(rectify=...) or rectified pairs and no
   rectification, one process per setting; the caller alternates the processes:

    python tools/prof_stereo_rectify.py e2e --rectify 0|1 [--steps 150] [--warmup 20]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, CALLS = 5, 30
W, H = 640, 480
DIST = (-0.05004, 0.120012, -0.0006259, -0.00118, -0.063505)
RVEC_L, RVEC_R = (0.012, -0.017, 0.009), (-0.015, 0.011, -0.013)
SGM = dict(max_disp=64, p2=100)


def rodrigues(r):
    import numpy as np
    r = np.asarray(r, np.float64); th = np.linalg.norm(r); k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _bgr(g):
    import numpy as np
    return np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=0), 255 - g], axis=-1))


def kernels():
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets, synth
    P, K_raw = (470.0, 470.0, 319.5, 239.5), (500.0, 500.0, 319.5, 239.5)
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    raw = synth.Scene3D(n_frames=3, w=W, h=H, K=P).raw_stereo_frame(1, 0.5, K_raw, DIST, rodrigues(RVEC_L), rodrigues(RVEC_R))
    maps = [V.rectify_map(K_raw, DIST, rodrigues(r), P, (W, H), (W, H)) for r in (RVEC_L, RVEC_R)]
    print("inside share of the maps: %.4f / %.4f" % (maps[0][1].mean(), maps[1][1].mean()))
    a, b = [torch.as_tensor(_bgr(g), device="cuda") for g in raw]
    ga, gb = [torch.as_tensor(g, device="cuda") for g in raw]
    ml, mr = [torch.as_tensor(m[0], device="cuda") for m in maps]
    ol, orr = torch.empty_like(a), torch.empty_like(b); gl, gr = torch.empty_like(ga), torch.empty_like(gb)
    il, ir = torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for _ in range(WARM + CALLS):
        ops.rectify(a, ml, b, mr, out_left=ol, out_right=orr, inside_left=il, inside_right=ir)
    torch.cuda.synchronize()
    for _ in range(WARM + CALLS):
        ops.rectify(a, ml, out_left=ol)
    torch.cuda.synchronize()
    for _ in range(WARM + CALLS):
        ops.rectify(ga, ml, gb, mr, out_left=gl, out_right=gr)
    torch.cuda.synchronize()
    disp = torch.empty((H, W), dtype=torch.float32, device="cuda"); stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    for _ in range(WARM + CALLS):
        ops.stereo_sgm(ol, orr, out=disp, stats=stats, **SGM)
    torch.cuda.synchronize()
    print("vido_stereo_sgm %s on the rectified pair: stats %s" % (SGM, stats.tolist()))


def parse(d):
    import csv, glob, statistics
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    rect = [r for r in rows if "k_rectify" in r["Kernel_Name"]]
    assert len(rect) == 3 * (WARM + CALLS), len(rect)
    lines = []; med = {}
    n = WARM + CALLS
    for i, (key, title) in enumerate((("pair", "two cameras, 3 channels, both inside planes (one launch)"), ("one", "one camera, 3 channels"), ("grey", "two cameras, 1 channel"))):
        t = [dur(r) for r in rect[i * n + WARM:(i + 1) * n]]
        med[key] = statistics.median(t)
        lines.append("vido_rectify, %s: kernel time per call, us: median %.1f min %.1f max %.1f over %d calls (%s)" % (title, med[key], min(t), max(t), len(t), rect[i * n]["Kernel_Name"].split("(")[0]))
    sgm = [r for r in rows if "k_sgm_" in r["Kernel_Name"]]
    per = len(sgm) // n
    assert per * n == len(sgm), len(sgm)
    t = [sum(dur(r) for r in sgm[k * per:(k + 1) * per]) for k in range(WARM, n)]
    med["sgm"] = statistics.median(t)
    lines.append("vido_stereo_sgm, max_disp 64, p2 100, on the rectified pair: %d launches per call; kernel time per call, us: median %.1f min %.1f max %.1f" % (per, med["sgm"], min(t), max(t)))
    traffic = 2 * (W * H * 8 + W * H * 3 * 2 + W * H) / 1e6
    print("%d x %d, one MI355X, rocprofv3 kernel trace, one process: vido_rectify of a 3-channel pair %.1f us per call (about %.1f MB of map, source, destination and inside "
          "traffic: %.0f GB/s) = %.3f of vido_stereo_sgm (%.1f us)" % (W, H, med["pair"], traffic, traffic / med["pair"] * 1e3, med["pair"] / med["sgm"], med["sgm"]))
    print("\n".join(lines))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rectify", type=int, default=0); ap.add_argument("--steps", type=int, default=150); ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System
    from bench import write_settings                                  # the bench's settings for its clip
    from concurrent.futures import ThreadPoolExecutor
    n_total = a.warmup + a.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5)          # its own camera is the rectified one; the raw cameras are a little longer and turned
    K_raw = (scene.K[0] / 0.94, scene.K[1] / 0.94, scene.K[2], scene.K[3])
    RL, RR = rodrigues(RVEC_L), rodrigues(RVEC_R)
    def render(k):
        g, d, f, m = scene.frame(k)
        if a.rectify:
            left, right = scene.raw_stereo_frame(k, 0.5, K_raw, DIST, RL, RR)
        else:
            left, right = g, scene.stereo_frame(k, 0.5)[1]
        return synth.gray_to_bgr(left), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32), synth.gray_to_bgr(right)
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_stereo_rectify_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    rect = dict(left=dict(K=K_raw, dist=DIST, R=RL, P=scene.K), right=dict(K=K_raw, dist=DIST, R=RR, P=scene.K)) if a.rectify else None
    nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, depth_source="stereo", rectify=rect)
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
    print("depth_source stereo, rectify %s: %.1f frames/s over %d steps after %d (graphs: depth %s, detector %s)" % (
        "on (raw pairs pushed)" if a.rectify else "off (rectified pairs pushed)", a.steps / dt, a.steps, a.warmup, nodes.g_depth is not None, nodes.g_det is not None), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
