"""CPU measurement behind Verify.MaxHamming: Hamming distance between a static point's SEED descriptor (the ORB keypoint that started the
track) and the oracle's rBRIEF at the flow-predicted position in the next frames, on a synth.Scene3D clip, against the same distance when the flow carries a
common wrong displacement.  No GPU: oracle functions only.  Prints the histograms and a threshold sweep (profiles/r8/descriptor_verify.txt keeps a run).

    python tools/measure_descriptor_verify.py [--frames 30] [--seed 3]
"""
import argparse
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as O                      # noqa: E402
from vido_slam_amd import synth                       # noqa: E402

EDGE = 19
POPCNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def describe(p, levels, blurred, xy, level, scale):
    """Oracle descriptor at lrintf(xy / scale[level]) of `level`, or None outside the extractor's margin (what vido_orb_describe_points computes)."""
    x = int(np.rint(np.float32(xy[0]) / np.float32(scale[level]))); y = int(np.rint(np.float32(xy[1]) / np.float32(scale[level])))
    h, w = levels[level].shape
    if not (EDGE <= x < w - EDGE and EDGE <= y < h - EDGE):
        return None
    return O.brief(blurred[level], x, y, O.ic_angle(levels[level], x, y, p))


def hist(d, step=16):
    h, _ = np.histogram(d, bins=np.arange(0, 257 + step, step))
    return " ".join("%5d" % v for v in h[:256 // step])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30); ap.add_argument("--seed", type=int, default=3); ap.add_argument("--every", type=int, default=3)
    a = ap.parse_args()
    p = O.orb_params(); scale = [p.scale[l] for l in range(8)]
    scene = synth.Scene3D(n_frames=a.frames, seed=a.seed, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    wrong = [(8, 0), (0, -8), (12, -9), (16, -12), (24, -18)]
    tracks = []                                        # [x, y, level, seed descriptor, age]
    true_d = {}; true_lv = {}; bad_d = {w: [] for w in wrong}; bad_lv = {w: {} for w in wrong}
    for k in range(a.frames):
        g, depth, flow, mask = scene.frame(k)
        levels = O.orb_pyramid(p, g); blurred = [O.gaussian_blur7(l) for l in levels]
        if k > 0:
            for t in tracks:                           # the seed against this frame at the predicted position, and at the predicted position + a wrong displacement
                d = describe(p, levels, blurred, (t[0], t[1]), t[2], scale)
                if d is None:
                    continue
                dist = int(POPCNT[d ^ t[3]].sum())
                true_d.setdefault(min(t[4], 20), []).append(dist); true_lv.setdefault(t[2], []).append(dist)
                for w in wrong:
                    dw = describe(p, levels, blurred, (t[0] + w[0], t[1] + w[1]), t[2], scale)
                    if dw is not None:
                        dd = int(POPCNT[dw ^ t[3]].sum()); bad_d[w].append(dd); bad_lv[w].setdefault(t[2], []).append(dd)
        kps, desc, _ = O.orb_extract(p, g)
        for i in range(0, len(kps), a.every):          # new tracks from this frame's static keypoints
            x, y = float(kps["x"][i]), float(kps["y"][i]); xi, yi = int(x), int(y)
            if mask[yi, xi] == 0 and 0 < depth[yi, xi] < 40:
                tracks.append([x, y, int(kps["octave"][i]), desc[i].copy(), 0])
        nxt = []
        for t in tracks:                               # p -> p + flow(p), as the tracker's lookup
            xi, yi = int(t[0]), int(t[1])
            if not (0 <= xi < scene.w and 0 <= yi < scene.h) or mask[yi, xi] != 0:
                continue
            nx, ny = t[0] + float(flow[yi, xi, 0]), t[1] + float(flow[yi, xi, 1])
            if 0 < nx < scene.w - 1 and 0 < ny < scene.h - 1:
                nxt.append([nx, ny, t[2], t[3], t[4] + 1])
        tracks = nxt
    print("clip: synth.Scene3D(n_frames=%d, seed=%d), one moving object; seeds = every %d-th static ORB keypoint of every frame; bins of 16 over [0, 256)" % (a.frames, a.seed, a.every))
    print("bins:            " + " ".join("%5d" % b for b in range(0, 256, 16)))
    alltrue = np.concatenate([np.array(v) for v in true_d.values()])
    print("TRUE position    " + hist(alltrue) + "   n=%d median=%d p90=%d p99=%d" % (len(alltrue), np.median(alltrue), np.percentile(alltrue, 90), np.percentile(alltrue, 99)))
    for lo, hi in ((1, 1), (2, 5), (6, 12), (13, 20)):
        v = np.concatenate([np.array(true_d.get(ag, [])) for ag in range(lo, hi + 1)] or [np.zeros(0)])
        if len(v):
            print("  age %2d-%2d      " % (lo, hi) + hist(v) + "   n=%d median=%d p90=%d p99=%d" % (len(v), np.median(v), np.percentile(v, 90), np.percentile(v, 99)))
    for l in sorted(true_lv):
        v = np.array(true_lv[l]); print("  level %d        " % l + hist(v) + "   n=%d median=%d p90=%d" % (len(v), np.median(v), np.percentile(v, 90)))
    for w in wrong:
        v = np.array(bad_d[w])
        print("WRONG (%3d,%3d)  " % w + hist(v) + "   n=%d median=%d p10=%d p1=%d" % (len(v), np.median(v), np.percentile(v, 10), np.percentile(v, 1)))
        for l in sorted(bad_lv[w]):
            u = np.array(bad_lv[w][l]); print("  level %d        " % l + hist(u) + "   n=%d median=%d p10=%d" % (len(u), np.median(u), np.percentile(u, 10)))
    print("threshold sweep (reject when dist > T): kept share of TRUE | rejected share of WRONG per displacement")
    for T in range(30, 121, 10):
        print("  T=%3d  kept %.3f | " % (T, np.mean(alltrue <= T)) + "  ".join("(%d,%d) %.3f" % (w[0], w[1], np.mean(np.array(bad_d[w]) > T)) for w in wrong))


if __name__ == "__main__":
    main()
