"""CPU measurement behind vido_dis_flow's defaults: the end-point error of the statement (tests/refimpl/dis_flow_np.py) against the exact flow of
synth.Scene3D and synth.convoy_scene, frame 1 -> 2.  Numpy and the statement only, no GPU.  profiles/r20/dis_flow_cpu.txt keeps a run.

    python tools/measure_dis_flow.py [--out profiles/r20/dis_flow_cpu.txt]

Only pixels whose true target lies at least 8 px inside the image are counted.  Per scene and class (static / object): median and p90 end-point error, the shares under
0.4 px (the tracker's RANSAC gate) and under 1 px, and the true flow's magnitude; the error by magnitude of the true flow; then sweeps of coarsest 2..5, iters 2 / 4 / 6 / 8
and max_shift 2 / 4 / 8 px around the defaults on the 640 x 480 scenes.

How the defaults follow from the numbers (the rules are fixed here, before any run of the tracker):
  coarsest      the knee plus one level, the knee being the smallest value after which the static share under 0.4 px gains less than 0.01 on BOTH 640 x 480 scenes.  One
                level of margin because the clips' largest flow (23-25 px) is what sets the knee and a level costs a quarter of the one below it; not more, because
                the coarsest level must still hold texture (min(w, h) >> coarsest >= 8 is the contract's floor).
  iters         the smallest value of the sweep after which the static share under 0.4 px gains less than 0.01 on both scenes.
  max_shift_q8  a convention, not a knee: half a patch (4 px = 1024).  The sweep shows what a tighter or wider window does to the rejected patches and the shares.
  min_eig       0: a flat patch keeps the coarser level's flow either way, and the densification already weights by the photometric error; no gate is measured here.
Where a sweep has no knee under its rule, the line says so."""
import argparse
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from vido_slam_amd import synth                       # noqa: E402
from refimpl import dis_flow_np as D                  # noqa: E402

BINS = ((0, 2), (2, 4), (4, 8), (8, 16), (16, 32), (32, 1e9))


def scenes():
    K2 = (721.5, 721.5, 620.5, 187.0); K3 = (157.0, 157.0, 100.0, 75.0)
    return [("Scene3D 640x480", synth.Scene3D()), ("convoy_scene 640x480", synth.convoy_scene(4)),
            ("Scene3D 1242x375", synth.Scene3D(w=1242, h=375, K=K2)), ("Scene3D 201x151", synth.Scene3D(w=201, h=151, K=K3))]


def pair(sc):
    g1, _, f1, m1 = sc.frame(1); g2 = sc.frame(2)[0]
    h, w = g1.shape
    Y, X = np.mgrid[0:h, 0:w]
    tx, ty = X + f1[..., 0], Y + f1[..., 1]
    inside = (tx >= 8) & (tx <= w - 1 - 8) & (ty >= 8) & (ty <= h - 1 - 8)
    return g1, g2, f1, m1, inside


def figures(e):
    return (float(np.median(e)), float((e < 0.4).mean()), float((e < 1).mean()), float(np.percentile(e, 90))) if len(e) else (float("nan"),) * 4


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    def say(s=""):
        print(s, flush=True); out.append(s)
    say("vido_dis_flow, the numpy statement against the renderer's exact flow, frame 1 -> 2; pixels whose true target is >= 8 px inside the image")
    say("defaults: coarsest %(coarsest)d iters %(iters)d max_shift_q8 %(max_shift_q8)d min_eig %(min_eig)d" % D.DEFAULTS)
    say()
    say("1. at the defaults (coarsest lowered to the contract's floor min(w, h) >> coarsest >= 8 where the frame is smaller)")
    say("%-22s %-7s %9s %10s %8s %8s %8s   %s   %s" % ("scene", "class", "pixels", "median px", "< 0.4", "< 1", "p90 px", "true |flow| median / p99 px", "stats kept flat rejected steps; seconds"))
    data = {}
    for name, sc in scenes():
        g1, g2, f1, m1, inside = pair(sc)
        L = D.DEFAULTS["coarsest"]
        while (min(g1.shape) >> L) < 8:
            L -= 1
        t = time.time()
        flow, q8, stats = D.dis_flow(g1, g2, **dict(D.DEFAULTS, coarsest=L))
        dt = time.time() - t
        epe = np.hypot(flow[..., 0] - f1[..., 0], flow[..., 1] - f1[..., 1]); mag = np.hypot(f1[..., 0], f1[..., 1])
        data[name] = (g1, g2, f1, m1, inside, epe, mag)
        for cls, sel in (("static", inside & (m1 == 0)), ("object", inside & (m1 > 0))):
            med, s04, s1, p90 = figures(epe[sel])
            say("%-22s %-7s %9d %10.3f %8.3f %8.3f %8.2f   %6.1f / %5.1f   %s" % (name, cls, sel.sum(), med, s04, s1, p90, np.median(mag[sel]), np.percentile(mag[sel], 99),
                                                                              "coarsest %d: %s; %.1f s" % (L, stats.tolist(), dt) if cls == "static" else ""))
    say()
    say("2. static pixels by magnitude of the true flow: pixels, median px, share < 0.4 px")
    for name in list(data)[:2]:
        g1, g2, f1, m1, inside, epe, mag = data[name]
        row = []
        for lo, hi in BINS:
            sel = inside & (m1 == 0) & (mag >= lo) & (mag < hi)
            row.append("%s px: %d %.2f %.2f" % ("%g-%g" % (lo, hi) if hi < 1e9 else ">= %g" % lo, sel.sum(), *figures(epe[sel])[:2]) if sel.sum() else "%g-: 0" % lo)
        say("%-22s %s" % (name, " | ".join(row)))
    say()
    say("3. sweeps around the defaults, 640 x 480: static median px, share < 0.4 px, share < 1 px | object the same | rejected patches")
    sweeps = (("coarsest", (2, 3, 4, 5)), ("iters", (2, 4, 6, 8)), ("max_shift_q8", (512, 1024, 2048)))
    for key, values in sweeps:
        gains = {}
        for name in list(data)[:2]:
            g1, g2, f1, m1, inside = data[name][:5]
            prev = None
            for v in values:
                flow, q8, stats = D.dis_flow(g1, g2, **dict(D.DEFAULTS, **{key: v}))
                epe = np.hypot(flow[..., 0] - f1[..., 0], flow[..., 1] - f1[..., 1])
                s, o = figures(epe[inside & (m1 == 0)]), figures(epe[inside & (m1 > 0)])
                say("%-22s %-13s %5d   static %.3f %.3f %.3f | object %.3f %.3f %.3f | rejected %d of %d" % (name, key, v, s[0], s[1], s[2], o[0], o[1], o[2], stats[2], stats[:3].sum()))
                if prev is not None:
                    gains.setdefault(v, []).append(s[1] - prev)
                prev = s[1]
        if key != "max_shift_q8":
            knee = None
            for i, v in enumerate(values[:-1]):                         # the smallest value after which no later step of the sweep gains 0.01 on either scene
                if all(max(gains[w]) < 0.01 for w in values[i + 1:]):
                    knee = v; break
            say("    rule (%s): %s" % (key, "the share under 0.4 px gains less than 0.01 on both scenes after %d%s" % (knee, "; the default is the knee plus one level" if key == "coarsest" else "")
                                       if knee is not None else "no knee inside the sweep: the last step still gains 0.01 on a scene"))
        else:
            say("    rule (max_shift_q8): a convention, half a patch; the rows above show what the window costs and buys")
        say()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
