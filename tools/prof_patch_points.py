"""Kernel time of vido_orb_patch_points beside vido_orb_describe_points at the same points (profiles/r16/patch_points.txt).

    rocprofv3 --kernel-trace -d DIR -o op --output-format csv -- python tools/prof_patch_points.py --op     # 3 alternating rounds of 20 launches per form, device-pointer form
    python tools/prof_patch_points.py --summarize DIR                                                       # median kernel time per launch from the trace

--op: 12 000 points spread over a 640 x 480 frame at level 0 (the tracker's dense object points: integer positions, no keypoint), after a warm-up launch of every form.
Each round launches, 20 times each and in this order: the verdict form of k_patch_points (reference patches in, sums and status out), its take form (patches out) and
k_describe_points with reference descriptors (distances out, the form Verify.Descriptor uses)."""
import argparse
import csv
import glob
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_POINTS = 12000
ROUNDS, PER_ROUND = 3, 20
FORMS = ("k_patch_points verdict", "k_patch_points take", "k_describe_points distances")


def op():
    import torch
    import vido_slam_amd as V
    ctx = V.Context(width=640, height=480, max_batch=1)
    ctx.orb_extract(V.synth.make_frame(640, 480, seed=3))
    r = np.random.default_rng(0)
    xyl = np.stack([r.integers(19, 640 - 19, N_POINTS), r.integers(19, 480 - 19, N_POINTS), np.zeros(N_POINTS, np.int64)], 1).astype(np.int32)
    own = ctx.orb_patch_points(0, xyl)[0]
    ref = np.clip(own.astype(np.int32) + r.integers(-12, 13, own.shape), 0, 255).astype(np.uint8)
    t_xyl = torch.from_numpy(xyl).cuda(); t_ref = torch.from_numpy(ref).cuda(); t_rd = torch.from_numpy(r.integers(0, 256, (N_POINTS, 32), dtype=np.uint8)).cuda()
    t_patch = torch.empty((N_POINTS, 64), dtype=torch.uint8, device="cuda"); t_sums = torch.empty((N_POINTS, 3), dtype=torch.int32, device="cuda")
    t_st = torch.empty(N_POINTS, dtype=torch.int32, device="cuda"); t_dist = torch.empty(N_POINTS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    forms = (lambda: ctx.orb_patch_points_device(0, t_xyl.data_ptr(), N_POINTS, t_ref.data_ptr(), 1, V.host.PATCH_MIN_VAR, V.host.PATCH_MIN_ZNCC_Q10, None, t_sums.data_ptr(), t_st.data_ptr()),
             lambda: ctx.orb_patch_points_device(0, t_xyl.data_ptr(), N_POINTS, None, 1, 0, 0, t_patch.data_ptr()),
             lambda: ctx.orb_describe_points_device(0, t_xyl.data_ptr(), N_POINTS, t_rd.data_ptr(), None, None, t_dist.data_ptr()))
    for f in forms:                                        # warm-up: one launch of every form (the summary drops them)
        f()
    ctx.synchronize()
    for _ in range(ROUNDS):
        for f in forms:
            for _ in range(PER_ROUND):
                f()
            ctx.synchronize()
    st = t_st.cpu().numpy()
    print("points %d: status counts accepted %d rejected %d no texture %d invalid %d" % (N_POINTS, (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), (st == -1).sum()))
    ctx.close()


def summarize(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    seq = [(x["Kernel_Name"].split("(")[0], int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) for x in rows
           if x["Kernel_Name"].split("(")[0] in ("k_patch_points", "k_describe_points")]
    # launch order: [orb_patch_points host call of op(): 1 k_patch_points] [warm-up: patch, patch, describe] then ROUNDS x (20 patch verdict, 20 patch take, 20 describe)
    seq = seq[4:]
    assert len(seq) == ROUNDS * 3 * PER_ROUND, len(seq)
    t = {f: [] for f in FORMS}
    for rd in range(ROUNDS):
        for i, f in enumerate(FORMS):
            blk = seq[(rd * 3 + i) * PER_ROUND:(rd * 3 + i + 1) * PER_ROUND]
            assert all(name == ("k_describe_points" if i == 2 else "k_patch_points") for name, _ in blk)
            t[f].append([v for _, v in blk])
    print("kernel time per launch, us: %d points at level 0 of a 640 x 480 frame; %d launches per form in %d alternating rounds of %d" % (N_POINTS, ROUNDS * PER_ROUND, ROUNDS, PER_ROUND))
    for f in FORMS:
        allv = np.concatenate(t[f])
        print("  %-30s median %7.2f   (rounds: %s; min %.2f max %.2f)" % (f, np.median(allv) / 1e3, "  ".join("%.2f" % (np.median(v) / 1e3) for v in t[f]), allv.min() / 1e3, allv.max() / 1e3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true"); ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.op:
        op()
    if a.summarize:
        summarize(a.summarize)
