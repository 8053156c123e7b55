"""Kernel time of vido_orb_patch_search beside vido_orb_patch_points' verdict form at the same points (profiles/r17/patch_search.txt).

    rocprofv3 --kernel-trace -d DIR -o op --output-format csv -- python tools/prof_patch_search.py --op     # 3 alternating rounds of 20 launches per form, device-pointer form
    python tools/prof_patch_search.py --summarize DIR                                                       # median kernel time per launch from the trace

--op: points spread over a 640 x 480 frame at level 0 of the blurred pyramid (the tracker's dense object points: integer positions), references = the level's own patch
3 px away with noise, after a warm-up launch of every form.  Each round launches, 20 times each and in this order: k_patch_search at 1 000 points radius 8, 1 000 points
radius 16, 12 000 points radius 8, 12 000 points radius 16, then k_patch_points' verdict form at 12 000 points.

The floor printed beside the medians is the kernel's own work, not a bound on a better algorithm: per point and candidate 64 multiply-adds for S12, 64 for S22 and 64 adds
for S2 (sixteen 4-byte dot products each), i.e. 192 (2 R + 1)^2 byte operations per point, against the chip's dense 8-bit dot-product rate; and the bytes that must move,
(2 R + 8)^2 window bytes + 76 in + 32 out per point, against the HBM rate."""
import argparse
import csv
import glob
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, PER_ROUND = 3, 20
CASES = ((1000, 8), (1000, 16), (12000, 8), (12000, 16))
FORMS = tuple("k_patch_search %5d points radius %2d" % c for c in CASES) + ("k_patch_points verdict 12000 points",)
DOT4_PER_S = 256 * 4 * 16 * 2.4e9              # 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz, one 4-byte dot product per lane and clock
HBM_BYTES_PER_S = 8e12


def op():
    import torch
    import vido_slam_amd as V
    ctx = V.Context(width=640, height=480, max_batch=1)
    ctx.orb_extract(V.synth.make_frame(640, 480, seed=3))
    r = np.random.default_rng(0); n_max = max(c[0] for c in CASES)
    xyl = np.stack([r.integers(24, 640 - 24, n_max), r.integers(24, 480 - 24, n_max), np.zeros(n_max, np.int64)], 1).astype(np.int32)
    off = xyl.copy(); off[:, 0] += 3
    own = ctx.orb_patch_points(0, off)[0]
    ref = np.clip(own.astype(np.int32) + r.integers(-6, 7, own.shape), 0, 255).astype(np.uint8)
    t_xyl = torch.from_numpy(xyl).cuda(); t_ref = torch.from_numpy(ref).cuda()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    t_dxy, t_sums, t_sec, t_st, t_stats = i32(n_max, 2), i32(n_max, 3), i32(n_max, 2), i32(n_max), i32(5)
    torch.cuda.synchronize()
    search = lambda n, rad: ctx.orb_patch_search_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), rad, 2, 1, V.host.PATCH_MIN_VAR, 976, 0, t_dxy.data_ptr(), t_sums.data_ptr(), t_sec.data_ptr(),
                                                        t_st.data_ptr(), t_stats.data_ptr())
    forms = [(lambda n=n, rad=rad: search(n, rad)) for n, rad in CASES]
    forms.append(lambda: ctx.orb_patch_points_device(0, t_xyl.data_ptr(), n_max, t_ref.data_ptr(), 1, V.host.PATCH_MIN_VAR, V.host.PATCH_MIN_ZNCC_Q10, None, t_sums.data_ptr(), t_st.data_ptr()))
    for f in forms:                                        # warm-up: one launch of every form (the summary drops them)
        f()
    ctx.synchronize()
    for _ in range(ROUNDS):
        for f in forms:
            for _ in range(PER_ROUND):
                f()
            ctx.synchronize()
    search(n_max, 8); ctx.synchronize()
    print("points %d radius 8: stats found %d not found %d no texture %d ambiguous %d invalid %d" % ((n_max,) + tuple(t_stats.cpu().numpy().tolist())))
    ctx.close()


def summarize(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    seq = [(x["Kernel_Name"].split("(")[0], int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) for x in rows if x["Kernel_Name"].split("(")[0] in ("k_patch_search", "k_patch_points")]
    # launch order: [orb_patch_points host call of op(): 1 k_patch_points] [warm-up: 4 search, 1 points] then ROUNDS x (4 x 20 search, 20 points) [the closing search]
    seq = seq[6:-1]
    nf = len(FORMS)
    assert len(seq) == ROUNDS * nf * PER_ROUND, len(seq)
    t = {f: [] for f in FORMS}
    for rd in range(ROUNDS):
        for i, f in enumerate(FORMS):
            blk = seq[(rd * nf + i) * PER_ROUND:(rd * nf + i + 1) * PER_ROUND]
            assert all(name == ("k_patch_points" if i == nf - 1 else "k_patch_search") for name, _ in blk)
            t[f].append([v for _, v in blk])
    print("kernel time per launch, us: level 0 of a 640 x 480 frame; %d launches per form in %d alternating rounds of %d" % (ROUNDS * PER_ROUND, ROUNDS, PER_ROUND))
    for i, f in enumerate(FORMS):
        allv = np.concatenate(t[f])
        floor = ""
        if i < len(CASES):
            n, rad = CASES[i]; cand = (2 * rad + 1) ** 2
            floor = "   floor: %.2f us of dot products (%d candidates x 48 per point), %.2f us of bytes" % (n * cand * 48 / DOT4_PER_S * 1e6, cand, n * ((2 * rad + 8) ** 2 + 108) / HBM_BYTES_PER_S * 1e6)
        print("  %-40s median %8.2f   (rounds: %s; min %.2f max %.2f)%s" % (f, np.median(allv) / 1e3, "  ".join("%.2f" % (np.median(v) / 1e3) for v in t[f]), allv.min() / 1e3, allv.max() / 1e3, floor))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true"); ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.op:
        op()
    if a.summarize:
        summarize(a.summarize)
