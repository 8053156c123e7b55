"""CPU measurement behind Verify.ObjectRecoverRadius / Excl / MinZncc / PeakRatio: the search of vido_orb_patch_search
(tests/refimpl/patch_search_np.py) for the 8 x 8 patch a dense object point carries from the blurred level 0 of frame k, in frame k + 1 around a WRONG prediction: the
rendered (exact) correspondence, rounded as the tracker rounds it, displaced by 2, 4, 8 and 12 px (along +x, +y, -x, -y in turn, one direction per point).  The population
is what the tracker would hand to the search: points with texture (PatchMinStd) whose patch Verify.ObjectPatch rejects at the displaced position (PatchMinZncc).  Per
displacement and radius 4 / 8 / 12 / 16 it gives the share re-found within 1 px of the rounded truth ("right"), the share accepted on another pixel ("wrong") and the share
not found, as functions of the gate, of excl and of the peak ratio.  No GPU: the oracle's blur and numpy only.  profiles/r17/patch_recover.txt keeps a run.

    python tools/measure_patch_recover.py [--frames 12] [--seed 3]

The order among candidates is the statement's (cov^2 / var_cur, eligible candidates only, ties to the nearest); it is evaluated here in float64 over all candidates at
once, which can differ from the exact integer order only on a tie below 1e-16 relative: irrelevant to three-digit shares.

How the defaults follow from the numbers (the rule is fixed here, before any run of the tracker):
  Radius     a convention, not a knee: 8, the displacement DESIGN.md section 7 and the corrupted test clip call a wrong flow.  The table shows what a larger one costs
             (wrong share at every displacement, (2R + 1)^2 candidates) and that a displacement beyond the radius is never re-found.
  MinZncc    the highest gate of the sweep that, at the default radius with the peak test off, costs at most 0.03 of the right share at 8 px against the verification's
             own gate (PatchMinZncc).  Not a knee: the wrong share falls steadily with the gate and the right share with it; the rule fixes the price paid.  The row to read
             it against is the displacement BEYOND the radius (12 px at radius 8): there the truth is outside the window, every accepted match is wrong, and the gate
             is the only protection, which is why the search needs a tighter gate than the test of one position.
  Excl       a convention: 2, the half width of the ZNCC peak profiles/r16/patch_verify.txt shows (0.87 at 2 px); the sweep shows how little it matters at the gate.
  PeakRatio  0 (off) unless, at the chosen gate, some ratio of the sweep lowers the wrong share by more than it lowers the right share; the sweep decides."""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O                      # noqa: E402
from vido_slam_amd import synth                       # noqa: E402

DISPLACEMENTS = (2, 4, 8, 12)
RADII = (4, 8, 12, 16)
EXCLS = (1, 2, 3, 4)
GATES = (768, 832, 896, 920, 944, 960, 976, 992, 1008)
RATIOS = (0, 717, 819, 870, 922, 973)                  # 0 = off, then 0.70 0.80 0.85 0.90 0.95
OBJECTS = ((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),)
MIN_VAR, VERIFY_Q10 = 147456, 920                       # Verify.PatchMinStd 6, Verify.PatchMinZncc 920 / 1024 (profiles/r16/patch_verify.txt)
RMAX = 16
DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))


def patch_at(img, x, y):
    return img[y - 4:y + 4, x - 4:x + 4].astype(np.int64).reshape(64)


def score_map(img, cx, cy, a, s1):
    """(33, 33) cov and var_cur (int64) of the candidates around (cx, cy), and which of them lie wholly inside the image"""
    h, w = img.shape
    pad = np.zeros((2 * RMAX + 8, 2 * RMAX + 8), np.int64)
    x0, y0 = cx - RMAX - 4, cy - RMAX - 4
    xa, xb, ya, yb = max(x0, 0), min(x0 + pad.shape[1], w), max(y0, 0), min(y0 + pad.shape[0], h)
    if xa < xb and ya < yb:
        pad[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    win = np.lib.stride_tricks.sliding_window_view(pad, (8, 8)).reshape(2 * RMAX + 1, 2 * RMAX + 1, 64)
    s2 = win.sum(2)
    d = np.arange(-RMAX, RMAX + 1)
    inside = ((cy + d >= 4) & (cy + d + 3 < h))[:, None] & ((cx + d >= 4) & (cx + d + 3 < w))[None, :]
    return 64 * (win @ a) - s1 * s2, 64 * (win * win).sum(2) - s2 * s2, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12); ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    scene = synth.Scene3D(n_frames=a.frames, seed=a.seed, objects=OBJECTS)
    dd = np.arange(-RMAX, RMAX + 1); DY, DX = np.meshgrid(dd, dd, indexing="ij"); D2 = DX * DX + DY * DY
    # per (displacement, radius): rows of [err (Chebyshev distance of the best from the truth), zncc of the best, ratio zncc2 / zncc1 per excl ...]; err = -1: no best
    rows = {(d, R): [] for d in DISPLACEMENTS for R in RADII}
    n_tex = {d: 0 for d in DISPLACEMENTS}; n_rej = {d: 0 for d in DISPLACEMENTS}
    prev = None
    for k in range(a.frames):
        g, depth, flow, mask = scene.frame(k)
        blur = O.gaussian_blur7(g)
        h, w = blur.shape
        if prev is not None:
            pb, px, py, pf = prev
            for i in range(len(px)):
                if px[i] < 4 or px[i] + 3 >= w or py[i] < 4 or py[i] + 3 >= h:
                    continue
                ref = patch_at(pb, px[i], py[i]); s1 = int(ref.sum()); var_ref = int(64 * (ref * ref).sum() - s1 * s1)
                if var_ref < MIN_VAR:
                    continue
                tx, ty = int(np.rint(px[i] + pf[i, 0])), int(np.rint(py[i] + pf[i, 1]))
                if tx < 4 or tx + 3 >= w or ty < 4 or ty + 3 >= h:
                    continue
                for d in DISPLACEMENTS:
                    ox, oy = DIRS[i % 4]; cx, cy = tx + d * ox, ty + d * oy
                    cov, var, inside = score_map(blur, cx, cy, ref, s1)
                    c0, v0 = int(cov[RMAX, RMAX]), int(var[RMAX, RMAX])
                    if not inside[RMAX, RMAX] or v0 < MIN_VAR:
                        continue                                                   # Verify.ObjectPatch: invalid or no texture, the point is kept and never searched
                    n_tex[d] += 1
                    if c0 > 0 and c0 * c0 * 1024 * 1024 >= VERIFY_Q10 * VERIFY_Q10 * var_ref * v0:
                        continue                                                   # accepted where it is: not the search's business
                    n_rej[d] += 1
                    elig = inside & (var >= MIN_VAR) & (cov > 0)
                    score = np.where(elig, cov.astype(np.float64) ** 2 / np.maximum(var, 1), -1.0)
                    for R in RADII:
                        inR = (np.abs(DX) <= R) & (np.abs(DY) <= R)
                        s = np.where(inR, score, -1.0); m = s.max()
                        if m <= 0:
                            rows[d, R].append([-1, 0.0] + [0.0] * len(EXCLS)); continue
                        cand = np.flatnonzero(s.reshape(-1) == m)
                        j = cand[np.lexsort((DX.reshape(-1)[cand], DY.reshape(-1)[cand], D2.reshape(-1)[cand]))[0]]
                        by, bx = int(DY.reshape(-1)[j]), int(DX.reshape(-1)[j])
                        err = max(abs(bx + d * ox), abs(by + d * oy))                # the truth is at (-d ox, -d oy) from the centre
                        z1 = np.sqrt(m / var_ref)
                        rat = []
                        for e in EXCLS:
                            s2 = np.where(np.maximum(np.abs(DX - bx), np.abs(DY - by)) > e, s, -1.0).max()
                            rat.append(np.sqrt(s2 / m) if s2 > 0 else 0.0)
                        rows[d, R].append([err, z1] + rat)
        ys, xs = np.mgrid[0:scene.h:4, 0:scene.w:4]
        sel = mask[ys, xs] != 0
        px = xs[sel].astype(np.int64); py = ys[sel].astype(np.int64)
        prev = (blur, px, py, flow[py, px].astype(np.float64))
    for key in rows:
        rows[key] = np.array(rows[key], np.float64).reshape(-1, 2 + len(EXCLS))

    def shares(T, q10, excl, ratio):
        """right, wrong, not found: found = a best that passes the gate and, with the peak test on, whose runner-up outside excl stays at or below ratio"""
        found = (T[:, 0] >= 0) & (T[:, 1] >= q10 / 1024.0)
        if ratio:
            found &= T[:, 2 + EXCLS.index(excl)] <= ratio / 1024.0
        right = found & (T[:, 0] <= 1); n = max(len(T), 1)
        return right.sum() / n, (found & ~right).sum() / n, (~found).sum() / n

    print("clip: synth.Scene3D(n_frames=%d, seed=%d, objects=%r); dense object samples (every 4th pixel of the mask) of frames 0 .. %d searched in the next frame;" % (a.frames, a.seed, OBJECTS, a.frames - 2))
    print("8 x 8 patches on the blurred level 0; centre = lrintf of the rendered correspondence + d px (one of +x, +y, -x, -y per point); min_var %d" % MIN_VAR)
    print("population: textured on both sides at the displaced centre AND rejected there by Verify.ObjectPatch (q10 %d)" % VERIFY_Q10)
    for d in DISPLACEMENTS:
        print("  displaced %2d px: textured %6d, rejected %6d (%.3f)" % (d, n_tex[d], n_rej[d], n_rej[d] / max(n_tex[d], 1)))
    print()
    print("right / wrong / not found by gate (excl 2, peak test off); rows: displacement, columns: radius")
    for q in GATES:
        print("  gate q10 %4d (%.3f)" % (q, q / 1024.0))
        for d in DISPLACEMENTS:
            print("    %2d px  " % d + "   ".join("R%-2d %.3f %.3f %.3f" % ((R,) + shares(rows[d, R], q, 2, 0)) for R in RADII))
    R0 = 8
    worst = {q: max(shares(rows[d, R0], q, 2, 0)[1] for d in DISPLACEMENTS) for q in GATES}
    right8 = {q: shares(rows[8, R0], q, 2, 0)[0] for q in GATES}
    gate = max(q for q in GATES if q <= VERIFY_Q10 or right8[VERIFY_Q10] - right8[q] <= 0.03)
    print()
    print("largest wrong share over the displacements at radius %d by gate: " % R0 + "  ".join("%d: %.3f" % (q, worst[q]) for q in GATES))
    print("right share at 8 px, radius %d by gate:                         " % R0 + "  ".join("%d: %.3f" % (q, shares(rows[8, R0], q, 2, 0)[0]) for q in GATES))
    print()
    print("at gate %d, radius %d: right / wrong / not found by excl and peak ratio (q10; 0 = off)" % (gate, R0))
    best_ratio = 0
    for e in EXCLS:
        for r in RATIOS:
            line = "  ".join("%2dpx %.3f %.3f %.3f" % ((d,) + shares(rows[d, R0], gate, e, r)) for d in DISPLACEMENTS)
            print("  excl %d ratio %4d   %s" % (e, r, line))
            if e == 2 and r:
                off = [shares(rows[d, R0], gate, 2, 0) for d in DISPLACEMENTS]; on = [shares(rows[d, R0], gate, 2, r) for d in DISPLACEMENTS]
                if sum(o[1] - p[1] for o, p in zip(off, on)) > sum(o[0] - p[0] for o, p in zip(off, on)) and not best_ratio:
                    best_ratio = r
    print()
    print("CHOSEN  Verify.ObjectRecoverRadius %d (convention)   Verify.ObjectRecoverMinZncc %.4f (min_zncc_q10 %d)   Verify.ObjectRecoverExcl 2 (convention)   Verify.ObjectRecoverPeakRatio %s" % (
        R0, gate / 1024.0, gate, ("%.4f (q10 %d)" % (best_ratio / 1024.0, best_ratio)) if best_ratio else "0 (off)"))
    for d in DISPLACEMENTS:
        r_, w_, nf = shares(rows[d, R0], gate, 2, best_ratio)
        print("  displaced %2d px (n = %d): right %.4f  wrong %.4f  not found %.4f" % (d, len(rows[d, R0]), r_, w_, nf))


if __name__ == "__main__":
    main()
