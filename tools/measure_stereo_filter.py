"""The statement of vido_stereo_filter (tests/refimpl/stereo_filter_np.py) on the statement of vido_stereo_sgm's output, against the exact disparity of
synth.Scene3D.stereo_frame and synth.convoy_scene, on the CPU: the evidence behind the filter's defaults.  Writes profiles/r26/stereo_filter_cpu.txt.

    python tools/measure_stereo_filter.py [--out profiles/r26/stereo_filter_cpu.txt]

The three pairs and the population are tools/measure_stereo_sgm.py's (true disparity below D - 1, counterpart at least 4 columns inside the right image); SGM runs at its
defaults.  Per cell of max_diff_q4 x min_region: `wrong removed` = the share of the population's valid pixels more than 1 px off that the filter turns into status 4,
`right lost` = the share of its valid pixels within 1 px that it turns into status 4.

The rule for the defaults, fixed before the numbers: among the cells that lose at most 1 % of the right pixels on EVERY pair, the one that removes the largest summed share
of wrong pixels; ties go to the larger max_diff_q4, then to the smaller min_region.  Should no cell qualify, the defaults are (16, 25)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_DIFFS = (4, 8, 16, 32)
MIN_REGIONS = (10, 25, 50, 100, 200, 400)
CAP = 0.01
FALLBACK = (16, 25)


def pairs(n=3):
    """[(name, left, right, true depth, bf)]: the first n of measure_stereo_sgm.py's three"""
    from vido_slam_amd import synth
    obj = ((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),)
    scenes = (("Scene3D 320 x 240 (seed 3), frame 1, baseline 0.3 m (bf 75)", lambda: synth.Scene3D(n_frames=3, w=320, h=240, K=(250, 250, 159.5, 119.5), seed=3, objects=obj), 0.3, 75.0),
              ("Scene3D 640 x 480 (seed 3), frame 1, baseline 0.5 m (bf 250)", lambda: synth.Scene3D(n_frames=3, seed=3, objects=obj), 0.5, 250.0),
              ("convoy_scene 640 x 480 (five objects), frame 1, baseline 0.5 m (bf 250)", lambda: synth.convoy_scene(4), 0.5, 250.0))
    out = []
    for name, make, base, bf in scenes[:n]:
        l, r, d, _ = make().stereo_frame(1, base)
        out.append((name, l, r, d, bf))
    return out


def populations(G, left, right, depth, bf):
    """SGM at its defaults -> (q4, status, right = valid and within 1 px, wrong = valid and more than 1 px off), both inside the tool's population"""
    disp, q4, status, _ = G.stereo_sgm(left, right, **G.DEFAULTS)
    w = left.shape[1]
    true = bf / depth.astype(np.float64)
    pop = (true < G.DEFAULTS["max_disp"] - 1) & (np.arange(w)[None, :] - true >= 4)
    ok = pop & (status == 0)
    err = np.abs(disp - true)
    return q4, status, ok & (err <= 1), ok & (err > 1)


def cell(F, q4, status, right, wrong, max_diff_q4, min_region):
    """-> (share of wrong pixels removed, share of right pixels lost)"""
    out = F.stereo_filter(q4, status, max_diff_q4=max_diff_q4, min_region=min_region)[1]
    gone = out == 4
    return (gone & wrong).sum() / max(int(wrong.sum()), 1), (gone & right).sum() / max(int(right.sum()), 1)


def choose(tables):
    """tables: per pair {(t, m): (removed, lost)} -> ((t, m), why)"""
    ok = [c for c in tables[0] if all(tb[c][1] <= CAP for tb in tables)]
    if not ok:
        return FALLBACK, "no cell loses at most %.0f %% of the right pixels on every pair: the fallback" % (100 * CAP)
    best = max(ok, key=lambda c: (sum(tb[c][0] for tb in tables), c[0], -c[1]))
    return best, "%d of %d cells lose at most %.0f %% of the right pixels on every pair; this one removes the largest summed share of wrong pixels (%.3f of 3)" % (
        len(ok), len(tables[0]), 100 * CAP, sum(tb[best][0] for tb in tables))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "stereo_filter_cpu.txt"))
    a = ap.parse_args()
    from refimpl import stereo_sgm_np as G, stereo_filter_np as F
    lines = ["tools/measure_stereo_filter.py — the numpy statement of vido_stereo_filter on the statement of vido_stereo_sgm (defaults %s) against rendered truth, CPU" % G.DEFAULTS,
             "cell: wrong removed % / right lost %   (wrong = valid and > 1 px off, right = valid and <= 1 px off, inside measure_stereo_sgm.py's population)"]
    tables = []
    for name, l, r, d, bf in pairs():
        q4, status, right, wrong = populations(G, l, r, d, bf)
        lines.append("%s: %d valid pixels in the population, %d of them wrong" % (name, int(right.sum() + wrong.sum()), int(wrong.sum())))
        lines.append("  max_diff_q4 \\ min_region " + "".join("%16d" % m for m in MIN_REGIONS))
        tb = {}
        for t in MAX_DIFFS:
            row = "  %-25s" % ("%d/16 px" % t)
            for m in MIN_REGIONS:
                tb[(t, m)] = cell(F, q4, status, right, wrong, t, m)
                row += "%16s" % ("%.1f / %.2f" % (100 * tb[(t, m)][0], 100 * tb[(t, m)][1]))
            lines.append(row); print(row, flush=True)
        tables.append(tb)
    best, why = choose(tables)
    lines.append("defaults by the rule: max_diff_q4 = %d, min_region = %d  (%s)" % (best[0], best[1], why))
    lines.append("stereo_filter_np.DEFAULTS = %s%s" % (F.DEFAULTS, "" if (F.DEFAULTS["max_diff_q4"], F.DEFAULTS["min_region"]) == best else "   <-- DIFFERS from the rule's choice"))
    print("\n".join(lines[-2:]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
