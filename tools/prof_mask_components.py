"""Connected-component labelling of a class label image (csrc/maskcc.hip): the measurements of profiles/r13/mask_components.txt.

1. Kernel time of HipOps.mask_components (a memset and seven launches) at 480x640, one process under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_mask_components.py kernels
    python tools/prof_mask_components.py parse DIR

   `kernels` runs the op on two images in three alternating rounds of 30 calls each: "blobs", the nine-ellipse label image of tools/prof_detect_every.py (nine values, the
   ellipses overpaint each other), and "convoy", the class image 3 * (gt > 0) of frame 0 of synth.convoy_scene (five cars, one value).  8-connected, min_area 1, id base
   0, cap 127, all outputs asked for.  `parse` prints median / min / max of the last 20 launches of each block, 60 per image, for the seven kernels and for whatever else ran
   between them (the runtime's fill kernel behind the memset of the area plane).

2. bench.py with the key off against the parent commit: the facade change must not move the flagship number.  bench.py builds its own networks, so each run is a process
   of its own; this tree and a checkout of the parent commit are started in turn, round by round, in one session:

    for r in 0 1 2: python bench.py --gpus 1 --steps 200 --warmup 20;  (parent checkout) python bench.py --gpus 1 --steps 200 --warmup 20

   The result lines are kept in the profile file as they were printed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGES = ("blobs", "convoy")
ROUNDS, CALLS, KEPT = 3, 30, 20
KERNELS = ("k_cc_local", "k_cc_seam", "k_cc_flatten", "k_cc_rowcount", "k_cc_scan", "k_cc_rank", "k_cc_relabel")


def images(H, W):
    import numpy as np
    import vido_slam_amd as V
    rng = np.random.RandomState(7)
    m = np.zeros((H, W), np.int32); yy, xx = np.mgrid[0:H, 0:W]
    for i in range(9):                                               # tools/prof_detect_every.py's blob image
        cy, cx, ry, rx = rng.randint(40, H - 40), rng.randint(40, W - 40), rng.randint(30, 90), rng.randint(40, 120)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = i + 1
    gt = V.synth.convoy_scene(2, w=W, h=H).frame(0)[3]
    return {"blobs": m, "convoy": (3 * (gt > 0)).astype(np.int32)}


def kernels():
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets
    H, W = 480, 640
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    imgs = {k: torch.from_numpy(v).cuda() for k, v in images(H, W).items()}
    out = torch.empty((H, W), dtype=torch.int32, device="cuda"); st = torch.zeros(4, dtype=torch.int32, device="cuda")
    cl = torch.zeros(127, dtype=torch.int64, device="cuda"); ar = torch.zeros(127, dtype=torch.int32, device="cuda")
    for rnd in range(ROUNDS):
        for name in IMAGES:
            for _ in range(CALLS):
                ops.mask_components(imgs[name], out=out, classes=cl, areas=ar, stats=st)
            torch.cuda.synchronize()
            print("round %d, %s: labelled %.3f of the pixels; stats (found, dropped, left out, kept) %s" % (rnd, name, float((imgs[name] > 0).float().mean()), st.tolist()))


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(f) == 1, f
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_cc_local"))
    last = max(i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("k_cc_relabel"))
    by = {}
    for r in rows[max(first - 1, 0):last + 1]:                      # (a call's fill comes just before its first launch)
        by.setdefault(r["Kernel_Name"].split("(")[0], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = ROUNDS * len(IMAGES) * CALLS
    sums = {name: 0.0 for name in IMAGES}
    for name, ns in by.items():
        if len(ns) % total:
            print("%s: %d launches in the window (not a multiple of the %d calls), all of them: median_ns %.0f" % (name, len(ns), total, statistics.median(ns))); continue
        per = len(ns) // total
        for ci, img in enumerate(IMAGES):
            b = []
            for rnd in range(ROUNDS):
                lo = ((rnd * len(IMAGES) + ci) * CALLS + (CALLS - KEPT)) * per
                b += ns[lo:lo + KEPT * per]
            print("%s %s x%d per call: median_ns %.0f min_ns %d max_ns %d n %d" % (name, img, per, statistics.median(b), min(b), max(b), len(b)))
            sums[img] += per * statistics.median(b)
    for img in IMAGES:
        print("sum of the medians, %s: %.1f us per call" % (img, sums[img] / 1000.0))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    else:
        sys.exit(__doc__)
