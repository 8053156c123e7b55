"""CPU measurement behind the Verify.Recover* defaults: how many of the static points that Verify.Descriptor rejects can be re-found by a windowed
descriptor search (the rule of vido_hamming_match_window) among the next frame's static ORB keypoints, and how many land on a wrong keypoint.  Same renderer, clip and
aging tracks as tools/measure_descriptor_verify.py.  No GPU: oracle functions only.  profiles/r15/descriptor_recover.txt keeps a run.

At every frame the seed of every track is compared with the frame at the flow-predicted position displaced by a common wrong displacement; the tracks whose distance
there exceeds Verify.MaxHamming (70) are the queries: seed descriptor, displaced position, seed level.  The train set is the frame's static keypoints.  A match is
CORRECT when the matched keypoint lies within 1.5 * scale[level] px of the undisplaced prediction, WRONG otherwise; NONE is every other status.  unique = 1 throughout,
as the tracker calls it.

    python tools/measure_descriptor_recover.py [--frames 14] [--every 4] [--seed 3]
"""
import argparse
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EDGE = 19
MAX_HAMMING = 70
POPCNT = np.array([bin(i).count("1") for i in range(256)], np.int32)
WRONG = [(16, -12), (8, 0), (24, -18)]
RADII = [16, 24, 32, 48]
LEVEL_TOLS = [0, 1]
MAX_DISTS = [30, 40, 50, 60, 70]
RATIOS = [None, (922, 1024), (819, 1024), (717, 1024)]          # off, 0.9, 0.8, 0.7 as round(1024 r) / 1024
CAP_WRONG = 0.05


def distance_matrix(q, t):
    """int32 [nq, nt] Hamming distances of uint8 [n, 32] descriptors"""
    out = np.empty((len(q), len(t)), np.int32)
    for a in range(0, len(q), 256):
        out[a:a + 256] = POPCNT[q[a:a + 256, None, :] ^ t[None, :, :]].sum(2)
    return out


def match_dense(D, q_xy, q_level, t_xy, t_level, radius, level_tol, max_dist, ratio, unique):
    """vido_hamming_match_window's rule on a precomputed distance matrix D (array form, for the sweep; tests/test_hamming_window_cpu.py holds it against the plain
    statement tests/refimpl/hamming_window_np.py).  Returns (idx, dist, dist2, status)."""
    nq, nt = D.shape
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, -1, np.int32); dist2 = np.full(nq, -1, np.int32); status = np.ones(nq, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist, dist2, status
    r = np.float32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(t_xy[None, :, 0] - q_xy[:, None, 0]) <= r) & (np.abs(t_xy[None, :, 1] - q_xy[:, None, 1]) <= r)
    if level_tol >= 0:
        ok &= np.abs(t_level[None, :].astype(np.int64) - q_level[:, None].astype(np.int64)) <= level_tol
    big = 1 << 20
    M = np.where(ok, D.astype(np.int32), np.int32(big))
    j1 = M.argmin(1); d1 = M[np.arange(nq), j1]                   # argmin: the first (lowest) j of the minimum
    M[np.arange(nq), j1] = big
    d2 = M.min(1)
    has1 = d1 < big; has2 = d2 < big
    dist[has1] = d1[has1]; dist2[has2] = d2[has2]
    status[:] = 0
    status[~has1] = 1
    status[has1 & (d1 > max_dist)] = 2
    if ratio is not None:
        num, den = ratio
        status[(status == 0) & has2 & ~(d1.astype(np.int64) * den < d2.astype(np.int64) * num)] = 3
    if unique:
        live = np.flatnonzero(status == 0)
        order = live[np.lexsort((live, d1[live], j1[live]))]      # by j, then dist, then i
        first = np.ones(len(order), bool); first[1:] = j1[order[1:]] != j1[order[:-1]]
        status[order[~first]] = 4
    idx[status == 0] = j1[status == 0]
    return idx, dist, dist2, status


def describe(O, p, levels, blurred, xy, level, scale):
    x = int(np.rint(np.float32(xy[0]) / np.float32(scale[level]))); y = int(np.rint(np.float32(xy[1]) / np.float32(scale[level])))
    h, w = levels[level].shape
    if not (EDGE <= x < w - EDGE and EDGE <= y < h - EDGE):
        return None
    return O.brief(blurred[level], x, y, O.ic_angle(levels[level], x, y, p))


def main():
    from oracle import pyoracle as O
    from vido_slam_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14); ap.add_argument("--seed", type=int, default=3); ap.add_argument("--every", type=int, default=4)
    a = ap.parse_args()
    p = O.orb_params(); scale = np.array([p.scale[l] for l in range(8)], np.float32)
    scene = synth.Scene3D(n_frames=a.frames, seed=a.seed, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    configs = [(r, lt, md, ra) for r in RADII for lt in LEVEL_TOLS for md in MAX_DISTS for ra in RATIOS]
    acc = {w: np.zeros((len(configs), 3), np.int64) for w in WRONG}       # correct, wrong, none
    kept = []                                                              # (w, D, q_xy, q_level, t_xy, t_level, truth, age) per frame and displacement
    miss = {w: [] for w in WRONG}                                          # distance of a wrong match from the truth, at the selected setting
    nq_total = {w: 0 for w in WRONG}; ntrain = []
    tracks = []
    for k in range(a.frames):
        g, depth, flow, mask = scene.frame(k)
        levels = O.orb_pyramid(p, g); blurred = [O.gaussian_blur7(l) for l in levels]
        kps, desc, _ = O.orb_extract(p, g)
        xi = kps["x"].astype(int); yi = kps["y"].astype(int)
        stat = np.flatnonzero((mask[yi, xi] == 0) & (depth[yi, xi] > 0) & (depth[yi, xi] < 40))
        t_xy = np.stack([kps["x"][stat], kps["y"][stat]], 1).astype(np.float32); t_level = kps["octave"][stat].astype(np.int32); t_desc = desc[stat]
        if k > 0:
            ntrain.append(len(stat))
            for w in WRONG:
                q = []
                for t in tracks:
                    dw = describe(O, p, levels, blurred, (t[0] + w[0], t[1] + w[1]), t[2], scale)
                    if dw is not None and int(POPCNT[dw ^ t[3]].sum()) > MAX_HAMMING:
                        q.append(t)
                if not q:
                    continue
                truth = np.array([[t[0], t[1]] for t in q], np.float32); q_xy = (truth + np.array(w, np.float32)).astype(np.float32)
                q_level = np.array([t[2] for t in q], np.int32); q_desc = np.stack([t[3] for t in q]); age = np.array([t[4] for t in q])
                D = distance_matrix(q_desc, t_desc)
                nq_total[w] += len(q)
                tol = 1.5 * scale[q_level]
                for c, (r, lt, md, ra) in enumerate(configs):
                    idx, _, _, st = match_dense(D, q_xy, q_level, t_xy, t_level, r, lt, md, ra, True)
                    m = st == 0
                    err = np.full(len(q), np.inf); err[m] = np.hypot(*(t_xy[idx[m]] - truth[m]).T)
                    good = m & (err <= tol)
                    acc[w][c] += (int(good.sum()), int((m & ~good).sum()), int((~m).sum()))
                kept.append((w, D.astype(np.uint16), q_xy, q_level, t_xy, t_level, truth, age))
        for i in stat[::a.every]:                          # new tracks from this frame's static keypoints
            tracks.append([float(kps["x"][i]), float(kps["y"][i]), int(kps["octave"][i]), desc[i].copy(), 0])
        nxt = []
        for t in tracks:                                   # p -> p + flow(p), as the tracker's lookup
            x, y = int(t[0]), int(t[1])
            if not (0 <= x < scene.w and 0 <= y < scene.h) or mask[y, x] != 0:
                continue
            nx, ny = t[0] + float(flow[y, x, 0]), t[1] + float(flow[y, x, 1])
            if 0 < nx < scene.w - 1 and 0 < ny < scene.h - 1:
                nxt.append([nx, ny, t[2], t[3], t[4] + 1])
        tracks = nxt

    print("clip: synth.Scene3D(n_frames=%d, seed=%d), one moving object; seeds = every %d-th static ORB keypoint of every frame, aging through the clip" % (a.frames, a.seed, a.every))
    print("queries: tracks whose seed is farther than %d from the frame at the displaced prediction; train set: the frame's static keypoints (%d .. %d per frame); unique = 1" % (
        MAX_HAMMING, min(ntrain), max(ntrain)))
    print("queries per displacement: " + "  ".join("(%d,%d) %d" % (w[0], w[1], nq_total[w]) for w in WRONG))
    print("shares: correct (within 1.5 * scale[level] px of the undisplaced prediction) / wrong / none")
    print("radius tol maxd ratio | " + " | ".join("(%3d,%3d) corr  wrong none" % w for w in WRONG))
    share = {w: acc[w] / max(nq_total[w], 1) for w in WRONG}
    for c, (r, lt, md, ra) in enumerate(configs):
        print("%6d %3d %4d %5s | " % (r, lt, md, "off" if ra is None else "%.1f" % (ra[0] / 1024.0)) +
              " | ".join("          %.3f %.3f %.3f" % tuple(share[w][c]) for w in WRONG))
    # selection: the highest correct share at (16, -12) with a wrong share <= CAP_WRONG there, among the radii that cover the largest displacement measured: a correct match
    # may lie 1.5 * scale[level] px from the truth, so the window has to reach the largest displacement component plus that tolerance at the coarsest level
    w0 = WRONG[0]; need = max(max(abs(w[0]), abs(w[1])) for w in WRONG) + 1.5 * float(scale[-1])
    elig = [c for c, cf in enumerate(configs) if cf[0] >= need]
    under = [c for c in elig if share[w0][c][1] <= CAP_WRONG]
    if under:
        best = max(under, key=lambda c: (share[w0][c][0], -share[w0][c][1]))
        print("selection: radius >= %.1f (the largest displacement component + 1.5 * scale[7]), wrong share at (%d,%d) <= %.2f, highest correct share:" % (need, w0[0], w0[1], CAP_WRONG))
    else:
        best = min(elig, key=lambda c: (share[w0][c][1], -share[w0][c][0]))
        print("selection: NO setting with radius >= %.1f keeps the wrong share at (%d,%d) under %.2f; the lowest wrong share:" % (need, w0[0], w0[1], CAP_WRONG))
    r, lt, md, ra = configs[best]
    print("  Verify.RecoverRadius %d  Verify.RecoverLevelTol %d  Verify.RecoverMaxHamming %d  Verify.RecoverRatio %s" % (r, lt, md, "0 (off)" if ra is None else "%.1f" % (ra[0] / 1024.0)))
    for w in WRONG:
        print("  at (%3d,%3d): correct %.3f wrong %.3f none %.3f" % ((w[0], w[1]) + tuple(share[w][best])))
    # the selected setting by age of the seed, and how far the wrong matches are from the truth
    ages = ((1, 1), (2, 5), (6, 12), (13, 99))
    tab = {(w, ag): np.zeros(3, np.int64) for w in WRONG for ag in ages}
    for w, D, q_xy, q_level, t_xy, t_level, truth, age in kept:
        idx, _, _, st = match_dense(D, q_xy, q_level, t_xy, t_level, r, lt, md, ra, True)
        m = st == 0; err = np.full(len(st), np.inf); err[m] = np.hypot(*(t_xy[idx[m]] - truth[m]).T)
        good = m & (err <= 1.5 * scale[q_level])
        miss[w] += list(err[m & ~good])
        for ag in ages:
            s = (age >= ag[0]) & (age <= ag[1])
            tab[(w, ag)] += (int((good & s).sum()), int((m & ~good & s).sum()), int((~m & s).sum()))
    print("the selected setting by age of the seed (frames since the keypoint that seeded the track):")
    for w in WRONG:
        for ag in ages:
            v = tab[(w, ag)]; n = int(v.sum())
            if n:
                print("  (%3d,%3d) age %2d-%2d  n=%6d  correct %.3f wrong %.3f none %.3f" % (w[0], w[1], ag[0], ag[1], n, v[0] / n, v[1] / n, v[2] / n))
        if miss[w]:
            print("  (%3d,%3d) wrong matches: median %.1f px from the truth, p90 %.1f px" % (w[0], w[1], np.median(miss[w]), np.percentile(miss[w], 90)))


if __name__ == "__main__":
    main()
