"""CPU measurement behind Verify.ObjectRecoverSubpixelIters / MaxShift / MinEig: the sub-pixel alignment of vido_orb_patch_refine
(tests/refimpl/patch_refine_np.py) at the points vido_orb_patch_search (tests/refimpl/patch_search_np.py, the tracker's defaults) re-finds within 1 px.  Renderer and
population are those of tools/measure_patch_recover.py: dense object samples of frame k, the 8 x 8 patch of the blurred level 0 at lrintf of the position, searched in
frame k + 1 around the rendered correspondence displaced by 8 px; textured on both sides and rejected there by Verify.ObjectPatch.  Unlike that tool the last position
carries a fraction (seeded, uniform in [-0.5, 0.5)^2), as a tracked point's does: the patch is cut at the rounded position, the truth is the fractional position plus the
rendered flow (bilinear) there.  No GPU: the oracle's blur and numpy only.  profiles/r19/patch_refine_cpu.txt keeps a run.

    python tools/measure_patch_refine.py [--frames 12] [--seed 3]

Distances to the true correspondence, in px:
    before   the re-found whole pixel, which is where Verify.ObjectRecover alone puts the point
    after    status 0: re-found pixel + q8 / 256 + the last position's fraction; any other status: the re-found pixel (the point is left as it was)
"refined" is the share of status 0, "worse" the share of the refined points that end farther from the truth than they started.

How the defaults follow from the numbers (the rules are fixed here, before any run of the tracker):
  Iters     a convention, not a knee: 6.  The sweep shows where the median over all points settles (the line "settled") and what further steps do: they move the
            refined points' tail a little and push a few more points out of the window.
  MaxShift  a convention, not a knee: 1.5 px.  The search is right within 1 px per axis and the fraction adds at most 0.5; the sweep shows what a tighter or wider window
            does to the shares of status 3.
  MinEig    the value of the sweep with the smallest p90 distance over ALL points, the smaller value on a tie.  A declined point keeps its whole pixel, so declining has
            a price; the gate pays only where the patches it declines (edge-like: they slide along the edge) would have ended farther away than that.  The table
            has a knee if some value above 0 brings the worse share below 0.01 while at least half of the points are still refined."""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O                      # noqa: E402
from vido_slam_amd import synth                       # noqa: E402
from refimpl import patch_points_np as PP             # noqa: E402
from refimpl import patch_search_np as S              # noqa: E402
from refimpl import patch_refine_np as R              # noqa: E402

OBJECTS = ((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),)
MIN_VAR, VERIFY_Q10 = 147456, 920                       # Verify.PatchMinStd 6, Verify.PatchMinZncc 920 / 1024 (profiles/r16/patch_verify.txt)
RADIUS, EXCL, REC_Q10, REC_RATIO = 8, 2, 976, 0         # Verify.ObjectRecover's defaults (profiles/r17/patch_recover.txt)
DISPLACED = 8
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))
ITERS = tuple(range(1, 9))
SHIFTS = (128, 256, 384, 512)
EIGS = (0, 3000, 10000, 30000, 100000, 300000, 1000000, 3000000)
IT0, SH0 = 6, 384


def bilinear(img, x, y):
    x0, y0 = int(np.floor(x)), int(np.floor(y)); ax, ay = x - x0, y - y0
    return (1 - ay) * ((1 - ax) * img[y0, x0] + ax * img[y0, x0 + 1]) + ay * ((1 - ax) * img[y0 + 1, x0] + ax * img[y0 + 1, x0 + 1])


def population(frames, seed):
    """per point: (blurred frame k + 1, re-found pixel, reference patch, fraction, truth)"""
    scene = synth.Scene3D(n_frames=frames, seed=seed, objects=OBJECTS)
    rng = np.random.RandomState(seed)
    pts = []; n_rej = n_found = 0; prev = None
    for k in range(frames):
        g, depth, flow, mask = scene.frame(k)
        blur = O.gaussian_blur7(g); h, w = blur.shape
        if prev is not None:
            pb, px, py, pflow = prev
            for i in range(len(px)):
                fr = rng.uniform(-0.5, 0.5, 2)
                if px[i] < 5 or px[i] + 4 >= w or py[i] < 5 or py[i] + 4 >= h:
                    continue
                ref = pb[py[i] - 4:py[i] + 4, px[i] - 4:px[i] + 4].reshape(64)
                lx, ly = px[i] + fr[0], py[i] + fr[1]                              # the last position; lrintf of it is (px, py)
                truth = np.array([lx + bilinear(pflow[..., 0], lx, ly), ly + bilinear(pflow[..., 1], lx, ly)])
                ox, oy = DIRS[i % 4]; cx, cy = int(np.rint(truth[0])) + DISPLACED * ox, int(np.rint(truth[1])) + DISPLACED * oy
                _, sm, st = PP.patch_points([blur], [(cx, cy, 0)], ref[None], MIN_VAR, VERIFY_Q10)
                if st[0] != 1:
                    continue                                                       # kept, or no evidence: never searched
                n_rej += 1
                st, dxy, _, _ = S.search_one([blur], cx, cy, 0, ref, RADIUS, EXCL, MIN_VAR, REC_Q10, REC_RATIO)
                if st != 0:
                    continue
                fx, fy = cx + dxy[0], cy + dxy[1]
                if max(abs(fx - int(np.rint(truth[0]))), abs(fy - int(np.rint(truth[1])))) > 1:
                    continue                                                       # a wrong match: not refinement's business
                n_found += 1
                pts.append((blur, fx, fy, ref, fr, truth))
        ys, xs = np.mgrid[0:scene.h:4, 0:scene.w:4]
        sel = mask[ys, xs] != 0
        prev = (blur, xs[sel].astype(np.int64), ys[sel].astype(np.int64), flow.astype(np.float64))
    return pts, n_rej, n_found


def run(pts, iters, shift, eig):
    """(before (n,), after (n,), status (n,), steps (n,))"""
    before = np.empty(len(pts)); after = np.empty(len(pts)); status = np.empty(len(pts), int); steps = np.empty(len(pts), int)
    for j, (blur, fx, fy, ref, fr, truth) in enumerate(pts):
        st, q8, _, it = R.refine_one([blur], fx, fy, 0, ref, iters, shift, eig)
        before[j] = np.hypot(fx - truth[0], fy - truth[1])
        after[j] = np.hypot(fx + q8[0] / 256.0 + fr[0] - truth[0], fy + q8[1] / 256.0 + fr[1] - truth[1]) if st == 0 else before[j]
        status[j] = st; steps[j] = it
    return before, after, status, steps


def line(tag, before, after, status):
    ok = status == 0; n = len(status)
    worse = (after[ok] > before[ok]).mean() if ok.any() else 0.0
    q = lambda v, p: np.percentile(v, p) if len(v) else float("nan")
    return "  %-22s refined %.3f  status2 %.3f  status3 %.3f  invalid %.3f | all points: median %.4f p90 %.4f p99 %.4f | refined only: median %.4f p90 %.4f p99 %.4f  worse %.4f" % (
        tag, ok.mean(), (status == 2).mean(), (status == 3).mean(), (status == -1).mean(), q(after, 50), q(after, 90), q(after, 99), q(after[ok], 50), q(after[ok], 90), q(after[ok], 99), worse), worse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12); ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    pts, n_rej, n_found = population(a.frames, a.seed)
    print("clip: synth.Scene3D(n_frames=%d, seed=%d, objects=%r); dense object samples (every 4th pixel of the mask) with a seeded fraction in [-0.5, 0.5)^2;" % (a.frames, a.seed, OBJECTS))
    print("8 x 8 patches on the blurred level 0 cut at the rounded last position; centre = lrintf of the true correspondence + %d px; rejected by Verify.ObjectPatch (q10 %d): %d;" % (DISPLACED, VERIFY_Q10, n_rej))
    print("re-found by the search (radius %d, excl %d, q10 %d, ratio %d) within 1 px of the rounded truth: %d = the population below" % (RADIUS, EXCL, REC_Q10, REC_RATIO, n_found))
    b0 = run(pts, 1, SH0, 0)[0]
    print("before (the re-found whole pixel): median %.4f p90 %.4f p99 %.4f px" % tuple(np.percentile(b0, (50, 90, 99))))
    print()
    print("by iters (max_shift_q8 %d, min_eig 0)" % SH0)
    med = {}
    for it in ITERS:
        b, af, st, steps = run(pts, it, SH0, 0)
        med[it] = np.median(af)
        print(line("iters %d" % it, b, af, st)[0] + "  mean steps %.2f" % steps.mean())
    print("settled: the median over all points is within 0.002 px of its value at 8 iterations from iters %d on" % min(it for it in ITERS if abs(med[it] - med[8]) <= 0.002))
    iters = IT0
    print()
    print("by max_shift_q8 (iters %d, min_eig 0)" % IT0)
    for sh in SHIFTS:
        b, af, st, _ = run(pts, IT0, sh, 0)
        print(line("max_shift_q8 %d" % sh, b, af, st)[0])
    print()
    print("by min_eig (iters %d, max_shift_q8 %d)" % (IT0, SH0))
    worse = {}; p90 = {}; refined = {}
    for e in EIGS:
        b, af, st, _ = run(pts, IT0, SH0, e)
        s, worse[e] = line("min_eig %d" % e, b, af, st)
        p90[e] = np.percentile(af, 90); refined[e] = (st == 0).mean()
        print(s)
    eig = min(EIGS, key=lambda e: (p90[e], e))
    knee = [e for e in EIGS if e > 0 and worse[e] < 0.01 and refined[e] >= 0.5]
    print()
    print("knee: " + ("min_eig %d brings the worse share below 0.01 with at least half of the points refined" % knee[0] if knee else
                      "none; no value above 0 brings the worse share below 0.01 while half of the points are still refined"))
    b, af, st, _ = run(pts, iters, SH0, eig)
    print("CHOSEN  Verify.ObjectRecoverSubpixelIters %d (convention)   Verify.ObjectRecoverSubpixelMaxShift 1.5 (max_shift_q8 %d, convention)   Verify.ObjectRecoverSubpixelMinEig %d" % (iters, SH0, eig))
    print(line("chosen", b, af, st)[0])
    print("RATIO   median after / median before over the population at the chosen values: %.4f / %.4f = %.4f" % (np.median(af), np.median(b), np.median(af) / np.median(b)))


if __name__ == "__main__":
    main()
