"""CPU measurement behind Verify.PatchMinZncc / Verify.PatchMinStd: the integer ZNCC of vido_orb_patch_points (tests/refimpl/patch_points_np.py)
between the 8 x 8 patch of a dense object point on the blurred level 0 of frame k and the patch at its correspondence in frame k + 1, on a synth.Scene3D clip with one
textured moving object.  The correspondence is the rendered (exact) flow, rounded as the tracker rounds it (lrintf), and the same displaced by 2, 4, 8 and 20 px.  No GPU:
the oracle's blur and numpy only.  profiles/r16/patch_verify.txt keeps a run.

    python tools/measure_patch_verify.py [--frames 30] [--seed 3]

How the two defaults follow from the numbers (the rule is fixed here, before any run of the tracker):
  PatchMinStd  = the lowest whole grey level s at which the kept share of the true correspondences whose two patches both have std >= s stops rising (rises by less
                 than 0.002 to s + 1): below it the share is pulled down by patches that hold nothing but the texture's noise, whose ZNCC is arbitrary.
                 (The share has no plateau: it keeps rising slowly as points on the object's outline leave the population, so the 0.002 cut-off, not a knee, picks s.)
  PatchMinZncc = the highest Q10 value that keeps at least 0.95 of the true correspondences with texture (both stds >= PatchMinStd).
The two depend on each other, so the pair is iterated from ZNCC 0.5 until it repeats.
"Flat" patches are defined on the source, not on the measurement: the 12 x 12 block of the object's texture under the patch centre is one constant rectangle colour plus
the canvas's N(0, 2^2) noise (block std <= 3)."""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O                      # noqa: E402
from vido_slam_amd import synth                       # noqa: E402
from refimpl import patch_points_np as R              # noqa: E402

DISPLACEMENTS = (2, 4, 8, 20)
OBJECTS = ((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),)


def patches(img, x, y):
    """(n,64) int64 patches at integer centres, and their validity"""
    h, w = img.shape
    ok = (x >= 4) & (x + 3 < w) & (y >= 4) & (y + 3 < h)
    xs = np.where(ok, x, 4); ys = np.where(ok, y, 4)
    dy, dx = np.meshgrid(np.arange(-4, 4), np.arange(-4, 4), indexing="ij")
    return img[ys[:, None] + dy.reshape(1, 64), xs[:, None] + dx.reshape(1, 64)].astype(np.int64), ok


def sums(a, b):
    s1, s2 = a.sum(1), b.sum(1)
    return 64 * (a * b).sum(1) - s1 * s2, 64 * (a * a).sum(1) - s1 * s1, 64 * (b * b).sum(1) - s2 * s2


def kept(cov, vr, vc, min_var, q):
    """share of status 0 among the points that are not status 2 (the statement's verdict, Python integers), and that population's size"""
    n = k = 0
    for c, a, b in zip(cov.tolist(), vr.tolist(), vc.tolist()):
        st = R.verdict(c, a, b, min_var, q)
        if st != 2:
            n += 1; k += st == 0
    return (k / n if n else 0.0), n


def dist(name, v):
    return "%-34s n=%6d  median %7.3f  p1 %7.3f  p10 %7.3f  p90 %7.3f" % (name, len(v), np.median(v), np.percentile(v, 1), np.percentile(v, 10), np.percentile(v, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30); ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    scene = synth.Scene3D(n_frames=a.frames, seed=a.seed, objects=OBJECTS)
    tex = scene.otex[0]
    T = {"cov": [], "vr": [], "vc": [], "flat": []}; D = {d: {"cov": [], "vr": [], "vc": []} for d in DISPLACEMENTS}
    prev = None
    for k in range(a.frames):
        g, depth, flow, mask = scene.frame(k)
        blur = O.gaussian_blur7(g)
        if prev is not None:
            pb, px, py, pf, flat = prev
            ref, ok_r = patches(pb, px, py)
            cx = np.rint(px + pf[:, 0]).astype(np.int64); cy = np.rint(py + pf[:, 1]).astype(np.int64)
            cur, ok_c = patches(blur, cx, cy)
            ok = ok_r & ok_c
            c, vr, vc = sums(ref[ok], cur[ok])
            T["cov"].append(c); T["vr"].append(vr); T["vc"].append(vc); T["flat"].append(flat[ok])
            for d in DISPLACEMENTS:
                for ox, oy in ((d, 0), (0, d), (-d, 0), (0, -d)):
                    cur, ok_c = patches(blur, cx + ox, cy + oy)
                    ok = ok_r & ok_c
                    c, vr, vc = sums(ref[ok], cur[ok])
                    D[d]["cov"].append(c); D[d]["vr"].append(vr); D[d]["vc"].append(vc)
        # this frame's dense object samples: every 4th pixel of the mask (the tracker's dense step), and whether the texture under each is flat
        ys, xs = np.mgrid[0:scene.h:4, 0:scene.w:4]
        sel = mask[ys, xs] != 0
        px = xs[sel].astype(np.int64); py = ys[sel].astype(np.int64)
        Twc = scene.poses[k]; ox_, oy_, oz_, vx, vy, vz = OBJECTS[0]
        cen = np.array([ox_ + vx * k, oy_ + vy * k, oz_ + vz * k])
        P = Twc[:3, 3] + (scene.rays[py, px] @ Twc[:3, :3].T) * depth[py, px][:, None].astype(np.float64)
        tx = np.floor(((P[:, 0] - cen[0] + 2) * 50.0) % (tex.shape[1] - 1)).astype(int); ty = np.floor(((P[:, 1] - cen[1] + 2) * 50.0) % (tex.shape[0] - 1)).astype(int)
        flat = np.zeros(len(px), bool)
        for i in range(len(px)):
            blk = tex[max(ty[i] - 6, 0):ty[i] + 6, max(tx[i] - 6, 0):tx[i] + 6]
            flat[i] = blk.std() <= 3.0
        prev = (blur, px, py, flow[py, px].astype(np.float64), flat)
    for key in ("cov", "vr", "vc", "flat"):
        T[key] = np.concatenate(T[key])
    for d in DISPLACEMENTS:
        for key in ("cov", "vr", "vc"):
            D[d][key] = np.concatenate(D[d][key])
    zn = lambda S: np.where((S["vr"] > 0) & (S["vc"] > 0), S["cov"] / np.sqrt(np.maximum(S["vr"].astype(np.float64) * S["vc"], 1.0)), 0.0)
    std_ref = np.sqrt(T["vr"]) / 64.0; std_cur = np.sqrt(T["vc"]) / 64.0
    print("clip: synth.Scene3D(n_frames=%d, seed=%d, objects=%r); dense object samples (every 4th pixel of the mask) of frames 0 .. %d against the next frame;" % (a.frames, a.seed, OBJECTS, a.frames - 2))
    print("8 x 8 patches on the blurred level 0 at lrintf of the rendered correspondence; displaced: the same + d px along +x, +y, -x, -y (pooled)")
    print()
    print("patch standard deviation (grey levels)")
    print(dist("  object points, all", std_ref))
    print(dist("  object points, textured source", std_ref[~T["flat"]]))
    print(dist("  object points, flat source", std_ref[T["flat"]]))
    print()
    print("ZNCC (float, for reading only; var = 0 counted as 0)")
    z = zn(T)
    print(dist("  true correspondence, all", z))
    print(dist("  true, textured source", z[~T["flat"]]))
    print(dist("  true, flat source", z[T["flat"]]))
    for s in (1, 2, 3, 4):
        m = (std_ref >= s) & (std_cur >= s)
        print(dist("  true, both stds >= %d" % s, z[m]))
    for d in DISPLACEMENTS:
        print(dist("  displaced %2d px, all" % d, zn(D[d])))
    print()

    def best_q(min_var):
        lo, hi = 0, 1024                                 # the kept share falls with q: the highest q that still keeps 0.95
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if kept(T["cov"], T["vr"], T["vc"], min_var, mid)[0] >= 0.95:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def best_s(q):
        ks = [kept(T["cov"], T["vr"], T["vc"], 4096 * s * s, q)[0] for s in range(0, 18)]
        for s in range(0, 17):
            if ks[s + 1] - ks[s] < 0.002:
                return s, ks
        return 16, ks

    q = 512; s = None
    for it in range(6):
        s2, ks = best_s(q); q2 = best_q(4096 * s2 * s2)
        print("iteration %d: at min_zncc_q10 = %4d the kept share by PatchMinStd 0 .. 12: %s -> PatchMinStd %d -> min_zncc_q10 %d" % (it, q, " ".join("%.3f" % v for v in ks[:13]), s2, q2))
        if (s2, q2) == (s, q):
            break
        s, q = s2, q2
    min_var = 4096 * s * s
    print()
    print("CHOSEN  Verify.PatchMinStd %d (min_var %d)   Verify.PatchMinZncc %.4f (min_zncc_q10 %d)" % (s, min_var, q / 1024.0, q))
    k, n = kept(T["cov"], T["vr"], T["vc"], min_var, q)
    print("true correspondences: %d, with texture %d (%.3f), kept share of those %.4f" % (len(T["cov"]), n, n / len(T["cov"]), k))
    print("rejected share per displacement (of the points with texture in both patches):")
    for d in DISPLACEMENTS:
        k, n = kept(D[d]["cov"], D[d]["vr"], D[d]["vc"], min_var, q)
        print("  %2d px: rejected %.4f   (n = %d of %d with texture)" % (d, 1.0 - k, n, len(D[d]["cov"])))
    print("threshold sweep at the chosen PatchMinStd: kept share of true | rejected share per displacement")
    for qq in (256, 512, 640, 768, 832, 896, 928, 960, 992):
        print("  q10 %4d (%.3f)  kept %.3f | " % (qq, qq / 1024.0, kept(T["cov"], T["vr"], T["vc"], min_var, qq)[0]) +
              "  ".join("%dpx %.3f" % (d, 1.0 - kept(D[d]["cov"], D[d]["vr"], D[d]["vc"], min_var, qq)[0]) for d in DISPLACEMENTS))


if __name__ == "__main__":
    main()
