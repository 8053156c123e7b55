"""Kernel time of the detector's paste launch: k_paste_instance (vido_mask_instance_image) against k_paste_label (vido_mask_label_image) on identical seeded inputs.
What profiles/r9/instance_label.txt records; one process per kernel and run, under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prof_instance_label.py run label|instance|instance_area
    python tools/prof_instance_label.py parse DIR

`run` launches the op 70 times on case A (100 clustered, heavily overlapping boxes at 480x640, soft 28x28 masks with entries exactly 0.5, 10 class-0 slots: the 100-box case of
tests/test_mask_instance_gpu.py), synchronises, then 70 times on case B (the static head's 100 slots with 5 live detections).  `parse` prints median / min / max of the last
60 launches of each block from DIR's kernel trace.  VIDO_LIB_VARIANT=<libvido_slam_hip.so of another build> measures that build's kernel (the parent commit's k_paste_label)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(which):
    import numpy as np
    import torch
    import vido_slam_amd as V
    from vido_slam_amd import nets
    H, W, n = 480, 640, 100
    ctx = V.Context(width=W, height=H, max_batch=1); ops = nets.HipOps(ctx)
    rng = np.random.RandomState(100 + H)
    cen = np.stack([rng.uniform(0.1 * W, 0.9 * W, 8), rng.uniform(0.1 * H, 0.9 * H, 8)], 1)
    c = cen[rng.randint(0, 8, n)] + rng.normal(0, 12, (n, 2)); wh = rng.uniform(20, 0.45 * H, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    m = rng.uniform(0.02, 0.98, (n, 1, 28, 28)).astype(np.float32); m[rng.rand(n, 1, 28, 28) < 0.1] = 0.5
    labels = rng.randint(1, 81, n).astype(np.int64); labels[rng.choice(n, n // 10, replace=False)] = 0
    A = (torch.from_numpy(m).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda())
    bB = np.zeros((n, 4), np.float32); lB = np.zeros(n, np.int64)
    bB[:5] = [[20, 150, 130, 260], [160, 170, 255, 265], [270, 180, 360, 262], [380, 170, 475, 265], [500, 150, 615, 262]]; lB[:5] = 3
    mB = rng.uniform(0.02, 0.98, (n, 1, 28, 28)).astype(np.float32); mB[:5] = 0.9
    B = (torch.from_numpy(mB).cuda(), torch.from_numpy(bB).cuda(), torch.from_numpy(lB).cuda())
    for case in (A, B):
        for _ in range(70):
            if which == "label":
                out = ops.mask_label_image(*case, H, W)
            else:
                out = ops.mask_instance_image(*case, H, W, areas=(which == "instance_area"))
        torch.cuda.synchronize()
    print("done", which, int((out[0] if isinstance(out, tuple) else out).sum()))


def parse(d):
    import csv, glob, statistics
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(f) == 1, f
    rows = [r for r in csv.DictReader(open(f[0])) if r["Kernel_Name"].startswith(("k_paste_label", "k_paste_instance"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    assert len(ns) == 140, len(ns)
    for name, blk in (("A_100boxes", ns[10:70]), ("B_5live", ns[80:140])):
        print("%s %s %s median_ns %.0f min_ns %d max_ns %d n %d" % (d, rows[0]["Kernel_Name"].split("(")[0], name, statistics.median(blk), min(blk), max(blk), len(blk)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in ("label", "instance", "instance_area"):
        run(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "parse":
        parse(sys.argv[2])
    else:
        sys.exit(__doc__)
