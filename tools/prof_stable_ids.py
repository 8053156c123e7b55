"""Instance ids that persist across frames: the two measurements of profiles/r11/stable_ids.txt.

1. Kernel time of the association (csrc/maskassoc.hip: a memset and three launches) at 480x640, one process under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_stable_ids.py kernels
    python tools/prof_stable_ids.py parse DIR

   `kernels` builds a blob image as tools/prof_detect_every.py does, with 5 and with 100 blobs, takes it as the previous label image (ids 1..n) and the same blobs shifted
   by the flow (5, 3) px with their slots permuted as the detector's image, and runs HipOps.mask_associate in three alternating rounds of 30 calls per instance count (the
   state is restored before every call, so every call does the same work).  `parse` prints median / min / max of the last 20 launches of each block, 60 per count, for
   the three kernels and for whatever else ran between them (the runtime's fill kernel behind the memset, the copy that restores the state).

2. End-to-end frames/s of pipeline.EndToEnd on the bench's clip (synth.convoy_scene, feed="given", device hand-over).  ONE set of networks per process: a second
   NetNodes in the process brings its own side stream and contexts, the streams then outnumber the hardware queues and networks that should overlap share a queue (measured:
   "off" 111 frames/s beside a second set against 137 alone).  So the configurations are separate processes, started in turn, round by round, in one session, so that drift
   of the machine falls on all alike:

    for r in 0 1 2: python tools/prof_stable_ids.py e2e --only off --rounds 1;  (parent checkout) ... --only off --rounds 1;  python tools/prof_stable_ids.py e2e --only ids --rounds 1

   off: NetNodes as bench.py builds it (stable_ids = False); ids: NetNodes(label_mode="instance", stable_ids=True), measured at detect_every 1 and 3 (ids1 / ids3).
   The parent commit is measured the same way from a CHECKOUT of the parent (its own package and library) with this file copied into its tools/: `e2e --only off`
   constructs NetNodes without the new arguments."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COUNTS = (5, 100)
ROUNDS, CALLS, KEPT = 3, 30, 20


def blob_pair(H, W, n, seed=7, shift=(5, 3)):
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    prev = np.zeros((H, W), np.int32); cur = np.zeros((H, W), np.int32)
    perm = rng.permutation(n)
    big = n <= 9
    for i in range(n):
        cy, cx = rng.randint(40, H - 40), rng.randint(40, W - 40)
        ry, rx = (rng.randint(30, 90), rng.randint(40, 120)) if big else (rng.randint(8, 30), rng.randint(10, 40))
        prev[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = i + 1
        cur[((yy - cy - shift[1]) / ry) ** 2 + ((xx - cx - shift[0]) / rx) ** 2 < 1] = 1 + perm[i]
    return prev, cur


def kernels():
    import numpy as np
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets
    H, W = 480, 640
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    cases = {}
    for n in COUNTS:
        prev, cur = blob_pair(H, W, n)
        state0 = np.zeros(768, np.int32); state0[0] = n; state0[257:257 + n] = 3
        cases[n] = (torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda(), torch.full((n,), 3, dtype=torch.int64, device="cuda"), torch.from_numpy(state0).cuda())
    out = torch.empty((H, W), dtype=torch.int32, device="cuda"); st = torch.zeros(4, dtype=torch.int32, device="cuda"); state = torch.zeros(768, dtype=torch.int32, device="cuda")
    for rnd in range(ROUNDS):
        for n in COUNTS:
            tp, tc, tk, s0 = cases[n]
            for _ in range(CALLS):
                state.copy_(s0)
                ops.mask_associate(tp, tc, state, classes=tk, hold=1, out=out, stats=st)
            torch.cuda.synchronize()
            print("round %d, %d instances: labelled %.3f of the pixels; stats (matched, fresh, lost, left out) %s" % (rnd, n, float((tc > 0).float().mean()), st.tolist()))


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(f) == 1, f
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_assoc_overlap"))
    last = max(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_assoc_relabel"))
    by = {}
    for r in rows[max(first - 2, 0):last + 1]:                      # (a call's state copy and fill come just before its first launch)
        by.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = ROUNDS * len(COUNTS) * CALLS
    for name, ns in by.items():
        if len(ns) % total:
            print("%s: %d launches in the window (not a multiple of the %d calls), all of them: median_ns %.0f" % (name, len(ns), total, statistics.median(ns))); continue
        per = len(ns) // total
        for ci, n in enumerate(COUNTS):
            b = []
            for rnd in range(ROUNDS):
                lo = ((rnd * len(COUNTS) + ci) * CALLS + (CALLS - KEPT)) * per
                b += ns[lo:lo + KEPT * per]
            print("%s %d instances x%d per call: median_ns %.0f min_ns %d max_ns %d n %d" % (name, n, per, statistics.median(b), min(b), max(b), len(b)))


def e2e(argv):
    import argparse
    import tempfile
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", required=True, choices=("off", "ids"), help="off: NetNodes without the new arguments (also in a checkout of the parent commit); ids: stable ids at detect_every 1 and 3")
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
    tmp = tempfile.mkdtemp(prefix="vido_stable_ids_")
    cfg = os.path.join(tmp, "settings.yaml"); write_settings(cfg, scene.K, W, H)
    configs = ["off"] if a.only == "off" else ["ids1", "ids3"]
    if a.only == "off":
        nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W)
    else:
        nodes = pipeline.NetNodes(V.Context(width=W, height=H, max_batch=1), H, W, label_mode="instance", stable_ids=True)
    res = {c: [] for c in configs}
    for rnd in range(a.rounds):
        for c in configs:
            if c != "off":
                nodes._set_detect_every(int(c[3:]))
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
            res[c].append(a.steps / dt)
            print("round %d %s: %.1f frames/s over %d steps (%d detector runs in %d frames)" % (rnd, c, a.steps / dt, a.steps, getattr(nodes, "detector_runs", 0) - runs0, n_total), flush=True)
    for c in configs:
        v = res[c]
        print("%s: frames/s %s  mean %.1f  min %.1f  max %.1f" % (c, " ".join("%.1f" % x for x in v), sum(v) / len(v), min(v), max(v)))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "e2e":
        e2e(sys.argv[2:])
    else:
        sys.exit(__doc__)
