"""CPU measurement behind vido_flow_consistency's defaults: what the forward-backward check keeps and rejects of the statement's flow
(tests/refimpl/dis_flow_np.py at its defaults, both directions; tests/refimpl/flow_consistency_np.py) against the exact flow of synth.Scene3D and synth.convoy_scene, frame
1 -> 2.  Numpy and the statements only, no GPU.  profiles/r21/flow_consistency_cpu.txt keeps a run.

    python tools/measure_flow_consistency.py [--out profiles/r21/flow_consistency_cpu.txt]

The scenes and the population are tools/measure_dis_flow.py's: only pixels whose true target lies at least 8 px inside the image are counted.  Per scene and class (static /
object), at the defaults: the share of the pixels with end-point error < 0.4 px (the tracker's RANSAC gate) that the check keeps, the share of the pixels with error >= 1 px
that it rejects, the share kept, and median, share under 0.4 px, share under 1 px and p90 of the kept pixels beside the same figures of all pixels.  Then the sweep of
alpha_q10 over 0 / 5 / 10 / 20 and beta_q16 over 4096 / 8192 / 16384 / 32768 / 65536 on every scene (static pixels): kept of the good, rejected of the bad, kept.

How the defaults follow from the numbers (the rule is fixed here, before the run):
  alpha_q10, beta_q16   the convention of Sundaram, Brox and Keutzer (ECCV 2010): |f + b|^2 < 0.01 (|f|^2 + |b|^2) + 0.5, i.e. alpha_q10 = 10 (10 / 1024 = 0.0098) and
                        beta_q16 = 32768 (0.5 px^2).  They are replaced only if another cell of the sweep rejects more of the >= 1 px pixels on BOTH 640 x 480 scenes while
                        keeping at least as many of the < 0.4 px pixels on both (static pixels, the tracker's pose population).  If no cell does, the line says so."""
import argparse
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from refimpl import dis_flow_np as D                  # noqa: E402
from refimpl import flow_consistency_np as F          # noqa: E402
from measure_dis_flow import scenes, pair, figures    # noqa: E402

ALPHAS = (0, 5, 10, 20)
BETAS = (4096, 8192, 16384, 32768, 65536)


def shares(epe, keep, sel):
    """(kept of the pixels under 0.4 px, rejected of the pixels at or over 1 px, kept) inside sel; nan where a population is empty"""
    good, bad = sel & (epe < 0.4), sel & (epe >= 1)
    frac = lambda a, b: float(a.sum()) / float(b.sum()) if b.sum() else float("nan")
    return frac(good & keep, good), frac(bad & ~keep, bad), frac(sel & keep, sel)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    def say(s=""):
        print(s, flush=True); out.append(s)
    say("vido_flow_consistency on the statement's flow against the renderer's exact flow, frame 1 -> 2; pixels whose true target is >= 8 px inside the image")
    say("flow defaults: coarsest %(coarsest)d iters %(iters)d max_shift_q8 %(max_shift_q8)d min_eig %(min_eig)d" % D.DEFAULTS + "; check defaults: alpha_q10 %(alpha_q10)d beta_q16 %(beta_q16)d" % F.DEFAULTS)
    say()
    say("1. at the defaults (coarsest lowered to the contract's floor min(w, h) >> coarsest >= 8 where the frame is smaller)")
    say("%-22s %-7s %9s | %9s %9s %7s | %-31s | %-31s | %s" % ("scene", "class", "pixels", "good kept", "bad rej.", "kept", "kept: median <0.4 <1 p90", "all: median <0.4 <1 p90", "status counts 0 1 2 3; seconds"))
    data = {}
    for name, sc in scenes():
        g1, g2, f1, m1, inside = pair(sc)
        L = D.DEFAULTS["coarsest"]
        while (min(g1.shape) >> L) < 8:
            L -= 1
        t = time.time()
        kw = dict(D.DEFAULTS, coarsest=L)
        fwd, bwd = D.dis_flow(g1, g2, **kw)[1], D.dis_flow(g2, g1, **kw)[1]
        status, marked, stats = F.flow_consistency(fwd, bwd)
        dt = time.time() - t
        flow = fwd.astype(np.float64) / 256
        epe = np.hypot(flow[..., 0] - f1[..., 0], flow[..., 1] - f1[..., 1])
        data[name] = (fwd, bwd, m1, inside, epe)
        keep = status == 0
        for cls, sel in (("static", inside & (m1 == 0)), ("object", inside & (m1 > 0))):
            gk, br, k = shares(epe, keep, sel)
            fk, fa = figures(epe[sel & keep]), figures(epe[sel])
            say("%-22s %-7s %9d | %9.3f %9.3f %7.3f | %7.3f %7.3f %7.3f %7.2f | %7.3f %7.3f %7.3f %7.2f | %s" % (name, cls, sel.sum(), gk, br, k, *fk, *fa,
                                                                                                             "%s; %.1f s" % (stats.tolist(), dt) if cls == "static" else ""))
    say()
    say("2. sweep, static pixels: good kept / bad rejected / kept per (alpha_q10, beta_q16)")
    cells = {}
    for name in data:
        fwd, bwd, m1, inside, epe = data[name]
        sel = inside & (m1 == 0)
        say(name)
        say("    %-10s " % "alpha_q10" + " ".join("%-19s" % ("beta_q16 %d" % b) for b in BETAS))
        for al in ALPHAS:
            row = []
            for be in BETAS:
                keep = F.flow_consistency(fwd, bwd, al, be)[0] == 0
                cells[(name, al, be)] = shares(epe, keep, sel)
                row.append("%.3f/%.3f/%.3f  " % cells[(name, al, be)])
            say("    %-10d " % al + " ".join(row))
    say()
    big = [n for n in data if "640x480" in n]
    d_al, d_be = F.DEFAULTS["alpha_q10"], F.DEFAULTS["beta_q16"]
    better = [(al, be) for al in ALPHAS for be in BETAS if (al, be) != (d_al, d_be)
              and all(cells[(n, al, be)][1] > cells[(n, d_al, d_be)][1] and cells[(n, al, be)][0] >= cells[(n, d_al, d_be)][0] for n in big)]
    if better:
        best = max(better, key=lambda c: sum(cells[(n, c[0], c[1])][1] for n in big))
        say("    rule: %d cell(s) reject more of the >= 1 px pixels on both 640 x 480 scenes while keeping at least as many of the < 0.4 px pixels on both: %s; the one that "
            "rejects most is alpha_q10 %d, beta_q16 %d — the defaults are to be replaced by it" % (len(better), better, best[0], best[1]))
    else:
        say("    rule: no cell of the sweep rejects more of the >= 1 px pixels on both 640 x 480 scenes while keeping at least as many of the < 0.4 px pixels on both: "
            "the defaults stay at the convention, alpha_q10 %d and beta_q16 %d" % (d_al, d_be))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
