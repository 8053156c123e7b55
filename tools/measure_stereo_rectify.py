"""vido_rectify_map / vido_rectify on the CPU: the figures of profiles/r27/stereo_rectify_cpu.txt, from the numpy statements alone (no GPU).

    python tools/measure_stereo_rectify.py [> profiles/r27/stereo_rectify_cpu.txt]

1. The rig test of tests/test_stereo_rectify_cpu.py: a 320 x 240 Scene3D pair seen through a raw rig (the KAIST distortion coefficients, about 1 degree of rotation per
   camera), SGM statement at max_disp = 64, p2 = 100: the share of the left-inside pixels with true disparity in [1, 63) that is valid and within 1 px, on the raw pair,
   on the pair rectified by the statement, and on the pair rendered directly in the rectified cameras.
2. The library's map (host code) against the statement's, entry by entry, for the three rigs of tests/refimpl/stereo_rectify_cases.py at 640 x 480.
3. The round trip of the map through vido_undistort_points, R and P, per rig: the largest and the mean distance from the pixel it started at."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import vido_slam_amd as V
    from refimpl import stereo_rectify_np as G
    from refimpl import stereo_rectify_cases as CASES
    import test_stereo_rectify_cpu as T
    r = T.rig_measure(V)
    print("rig: Scene3D(w=320, h=240, K=P, seed=3) frame 1, baseline 0.5 m, P = %s, K_raw = %s, dist = %s, R_left = Rodrigues(0.012, -0.017, 0.009), "
          "R_right = Rodrigues(-0.015, 0.011, -0.013); SGM statement max_disp = 64, p2 = 100" % (T.RIG["P"], T.RIG["K_raw"], CASES.KAIST_DIST))
    print("inside share of the maps: left %.4f, right %.4f (bar >= 0.85); population (left-inside, true disparity in [1, 63)): %d pixels" % (
        r["inside_left"], r["inside_right"], r["population"]))
    print("%-52s %-12s %s" % ("pair", "valid share", "valid and within 1 px of the truth"))
    for name, title in (("raw", "raw pair (bar <= 0.10)"), ("rectified", "raw pair rectified by the statement (bar >= 0.75)"), ("direct", "pair rendered in the rectified cameras")):
        print("%-52s %-12.4f %.4f" % (title, r[name + "_valid"], r[name]))
    for which in CASES.RIGS:
        cal = CASES.rig(640, 480, which)
        want, wins = G.rectify_map(src_size=(640, 480), dst_size=(640, 480), **cal)
        got, gins = V.rectify_map(src_size=(640, 480), dst_size=(640, 480), **cal)
        ok = wins.astype(bool)
        raw = want[ok].astype(np.float64) / 256.0
        und = V.undistort_points(raw.astype(np.float32), cal["K"], cal["dist"]).astype(np.float64)
        fx, fy, cx, cy = cal["K"]; fxp, fyp, cxp, cyp = cal["P"]
        n = np.stack([(und[:, 0] - cx) / fx, (und[:, 1] - cy) / fy, np.ones(len(und))], -1) @ np.asarray(cal["R"]).T
        v, u = np.nonzero(ok)
        err = np.hypot(n[:, 0] / n[:, 2] * fxp + cxp - u, n[:, 1] / n[:, 2] * fyp + cyp - v)
        print("rig %-6s 640 x 480: library map != statement map in %d of %d entries; inside %.4f; round trip through vido_undistort_points, R, P: max %.5f px, mean %.5f px "
              "(bar 0.01 px)" % (which, int((got != want).sum()), want.size, wins.mean(), err.max(), err.mean()))


if __name__ == "__main__":
    main()
