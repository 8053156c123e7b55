"""Kernel time of vido_orb_patch_refine (profiles/r19/patch_refine.txt).

    rocprofv3 --kernel-trace -d DIR -o op --output-format csv -- python tools/prof_patch_refine.py --op     # 3 alternating rounds of 20 launches per form, device-pointer form
    python tools/prof_patch_refine.py --summarize DIR                                                       # median kernel time per launch from the trace

--op: points spread over a 640 x 480 frame at level 0 of the blurred pyramid, references = the level bilinearly resampled up to 0.7 px away, with noise (what the tracker
hands over: a patch the search has put within a pixel), 6 iterations, window 1.5 px, min_eig 0, after a warm-up launch of every form.  Each round launches k_patch_refine
20 times each at 250, 1 000 and 12 000 points.

The floor printed beside the medians is the kernel's own arithmetic, not a bound on a better algorithm: per point and evaluated iterate 36 pixels x about 40 integer
operations (bilinear form, error, four products) and four wave reductions, against 256 CUs x 64 lanes at 2.4 GHz; and the bytes that must move, (7 + 2 C)^2 window bytes
+ 76 in + 32 out per point, against the HBM rate."""
import argparse
import csv
import glob
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, PER_ROUND = 3, 20
CASES = (250, 1000, 12000)
ITERS, MAX_SHIFT_Q8, MIN_EIG = 6, 384, 0
FORMS = tuple("k_patch_refine %5d points" % n for n in CASES)
LANE_OPS_PER_S = 256 * 64 * 2.4e9
HBM_BYTES_PER_S = 8e12


def op():
    import torch
    import vido_slam_amd as V
    ctx = V.Context(width=640, height=480, max_batch=1)
    ctx.orb_extract(V.synth.make_frame(640, 480, seed=3))
    L = ctx.orb_level(0, 0, blurred=True).astype(np.float64)
    r = np.random.default_rng(0); n_max = max(CASES)
    xyl = np.stack([r.integers(24, 640 - 24, n_max), r.integers(24, 480 - 24, n_max), np.zeros(n_max, np.int64)], 1).astype(np.int32)
    off = r.uniform(-0.7, 0.7, (n_max, 2))
    X = xyl[:, 0, None, None] - 4 + np.arange(8)[None, None, :] + off[:, 0, None, None]; Y = xyl[:, 1, None, None] - 4 + np.arange(8)[None, :, None] + off[:, 1, None, None]
    x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int); ax, ay = X - x0, Y - y0
    own = (1 - ay) * ((1 - ax) * L[y0, x0] + ax * L[y0, x0 + 1]) + ay * ((1 - ax) * L[y0 + 1, x0] + ax * L[y0 + 1, x0 + 1])
    ref = np.clip(np.rint(own + r.normal(0, 1.5, own.shape)), 0, 255).astype(np.uint8).reshape(n_max, 64)
    t_xyl = torch.from_numpy(xyl).cuda(); t_ref = torch.from_numpy(ref).cuda()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    t_q8, t_it, t_st, t_stats = i32(n_max, 2), i32(n_max), i32(n_max), i32(4); t_cost = torch.empty((n_max, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    refine = lambda n: ctx.orb_patch_refine_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), ITERS, MAX_SHIFT_Q8, MIN_EIG, 1, t_q8.data_ptr(), t_cost.data_ptr(), t_it.data_ptr(), t_st.data_ptr(),
                                                   t_stats.data_ptr())
    for n in CASES:                                        # warm-up: one launch of every form (the summary drops them)
        refine(n)
    ctx.synchronize()
    for _ in range(ROUNDS):
        for n in CASES:
            for _ in range(PER_ROUND):
                refine(n)
            ctx.synchronize()
    refine(n_max); ctx.synchronize()
    q8 = t_q8.cpu().numpy(); st = t_st.cpu().numpy(); ok = st == 0
    err = np.hypot(*(q8[ok] / 256.0 - off[ok]).T)
    print("points %d: stats refined %d declined %d left the window %d invalid %d; mean steps %.2f; distance of q8 from the resampling offset: median %.4f p90 %.4f px" % (
        (n_max,) + tuple(t_stats.cpu().numpy().tolist()) + (float(t_it.cpu().numpy().mean()), float(np.median(err)), float(np.percentile(err, 90)))))
    ctx.close()


def summarize(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    seq = [int(x["End_Timestamp"]) - int(x["Start_Timestamp"]) for x in rows if x["Kernel_Name"].split("(")[0] == "k_patch_refine"]
    # launch order: [warm-up: one per form] then ROUNDS x (forms x PER_ROUND) [the closing launch]
    nf = len(FORMS)
    seq = seq[nf:-1]
    assert len(seq) == ROUNDS * nf * PER_ROUND, len(seq)
    t = {f: [] for f in FORMS}
    for rd in range(ROUNDS):
        for i, f in enumerate(FORMS):
            t[f].append(seq[(rd * nf + i) * PER_ROUND:(rd * nf + i + 1) * PER_ROUND])
    print("kernel time per launch, us: level 0 of a 640 x 480 frame, iters %d max_shift_q8 %d min_eig %d; %d launches per form in %d alternating rounds of %d" % (
        ITERS, MAX_SHIFT_Q8, MIN_EIG, ROUNDS * PER_ROUND, ROUNDS, PER_ROUND))
    C_ = (MAX_SHIFT_Q8 + 255) >> 8
    for i, f in enumerate(FORMS):
        allv = np.concatenate(t[f]); n = CASES[i]
        floor = "   floor: %.3f us of lane operations (%d evaluations x 36 pixels x 40), %.3f us of bytes" % (
            n * (ITERS + 1) * 36 * 40 / LANE_OPS_PER_S * 1e6, ITERS + 1, n * ((7 + 2 * C_) ** 2 + 108) / HBM_BYTES_PER_S * 1e6)
        print("  %-30s median %8.2f   (rounds: %s; min %.2f max %.2f)%s" % (f, np.median(allv) / 1e3, "  ".join("%.2f" % (np.median(v) / 1e3) for v in t[f]), allv.min() / 1e3, allv.max() / 1e3, floor))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true"); ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.op:
        op()
    if a.summarize:
        summarize(a.summarize)
