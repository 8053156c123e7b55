"""The statement of vido_stereo_sgm (tests/refimpl/stereo_sgm_np.py) against the exact disparity of synth.Scene3D.stereo_frame and synth.convoy_scene, on the CPU: the
evidence behind the op's defaults (max_disp 128, p1 10, p2 120, uniqueness 10, lr_tol 1).  Writes profiles/r25/stereo_sgm_cpu.txt.

    python tools/measure_stereo_sgm.py [--out profiles/r25/stereo_sgm_cpu.txt]

Per run: the population is the pixels whose true disparity is below D - 1 and whose counterpart lies at least 4 columns inside the right image (x - true >= 4); `valid` is
the share of the population with status 0, `<= 1 px` the share of those within 1 px of the truth, `median` their median |error| in px, `wrong` the share of the population
that is valid AND more than 1 px off (what a consumer would take for a depth and should not).  The sweeps change one parameter at a time from the defaults on the
320 x 240 pair of tests/test_stereo_sgm_cpu.py; the full-size runs are at the defaults."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def score(G, left, right, depth, bf, **kw):
    p = {**G.DEFAULTS, **kw}
    t0 = time.perf_counter()
    disp, q4, status, stats = G.stereo_sgm(left, right, **p)
    dt = time.perf_counter() - t0
    h, w = left.shape
    true = bf / depth.astype(np.float64)
    pop = (true < p["max_disp"] - 1) & (np.arange(w)[None, :] - true >= 4)
    valid = pop & (status == 0)
    err = np.abs(disp[valid] - true[valid])
    return "valid %.4f  <= 1 px %.4f  median %.3f px  wrong %.4f  | population %.3f of the image, stats %s, %.1f s" % (
        valid.sum() / pop.sum(), (err <= 1).mean(), np.median(err), (err > 1).sum() / pop.sum(), pop.mean(), stats.tolist(), dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "stereo_sgm_cpu.txt"))
    a = ap.parse_args()
    from refimpl import stereo_sgm_np as G
    from vido_slam_amd import synth
    lines = ["tools/measure_stereo_sgm.py — the numpy statement of vido_stereo_sgm against rendered truth, CPU; defaults %s" % G.DEFAULTS]
    small = synth.Scene3D(n_frames=3, w=320, h=240, K=(250, 250, 159.5, 119.5), seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    l, r, d, _ = small.stereo_frame(1, 0.3)
    lines.append("Scene3D 320 x 240 (seed 3, one object), frame 1, baseline 0.3 m (bf 75), one parameter changed at a time:")
    sweeps = [("max_disp", (64, 96, 128)), ("p1", (0, 5, 10, 20, 40)), ("p2", (10, 60, 120, 240, 480)), ("uniqueness", (0, 5, 10, 20, 40)), ("lr_tol", (0, 1, 2, 255))]
    for key, values in sweeps:
        for v in values:
            kw = {"max_disp": 64, key: v}
            if kw.get("p1", G.DEFAULTS["p1"]) > kw.get("p2", G.DEFAULTS["p2"]):
                continue
            lines.append("  %-10s %4d%s  %s" % (key, v, " *" if G.DEFAULTS[key] == v else "  ", score(G, l, r, d, 75.0, **kw)))
            print(lines[-1], flush=True)
    lines.append("  (* = the default; max_disp is 64 in every other row of this block: the pair's largest disparity is 45 px)")
    full = synth.Scene3D(n_frames=3, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    l, r, d, _ = full.stereo_frame(1, 0.5)
    lines.append("Scene3D 640 x 480 (seed 3, one object), frame 1, baseline 0.5 m (bf 250), defaults:        " + score(G, l, r, d, 250.0))
    print(lines[-1], flush=True)
    lines.append("Scene3D 640 x 480, the same pair, uniqueness 5:                                          " + score(G, l, r, d, 250.0, uniqueness=5))
    print(lines[-1], flush=True)
    conv = synth.convoy_scene(4)
    l, r, d, _ = conv.stereo_frame(1, 0.5)
    lines.append("convoy_scene 640 x 480 (five objects), frame 1, baseline 0.5 m (bf 250), defaults:       " + score(G, l, r, d, 250.0))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
