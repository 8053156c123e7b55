"""Cost of Verify.Descriptor (profiles/r8/descriptor_verify.txt): tracks a synth.Scene3D clip with the option off and on and prints the tracker's own per-frame
times (vido_system_stats) and the verification counts.  Under `rocprofv3 --kernel-trace --stats -- python tools/prof_verify.py` the trace holds k_describe_points
(one launch per frame, all static points) beside k_orient_brief (one launch per frame, all keypoints).

    python tools/prof_verify.py [--frames 30]
"""
import argparse
import os
import sys
import tempfile
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vido_slam_amd as V                              # noqa: E402
from vido_slam_amd.system import System               # noqa: E402


def settings(path, scene, extra):
    fx, fy, cx, cy = scene.K
    with open(path, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (scene.w, scene.h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: 387.57\nCamera.fps: 10.0\nCamera.RGB: 0\nChooseData: 1\nDepthMapFactor: 1.0\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n")
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n" + extra)
    return path


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--frames", type=int, default=30); a = ap.parse_args()
    scene = V.synth.Scene3D(n_frames=a.frames, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = [scene.frame(k) for k in range(a.frames)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("off", ""), ("on", "Verify.Descriptor: 1\n"), ("off", ""), ("on", "Verify.Descriptor: 1\n")):
            slam = System(); slam.Init(settings(os.path.join(tmp, "s.yaml"), scene, extra), System.RGBD)
            tot, frm, chk, rej, keep = [], [], [], [], []
            for k, (g, d, f, m) in enumerate(frames):
                arrs = (g, np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)); keep.append(arrs)
                slam.TrackRGBD(*arrs, None, None, float(k), None, a.frames)
                st = slam.stats(); c, r = slam.verify_stats()
                if k >= 3:
                    tot.append(st["ms_total"]); frm.append(st["ms_frame"]); chk.append(c); rej.append(r)
            slam.close()
            print("Verify.Descriptor %-3s  frames 3..%d: ms_total median %.3f mean %.3f | ms_frame median %.3f mean %.3f | checked per frame %.0f, rejected %.1f" % (
                name, a.frames - 1, np.median(tot), np.mean(tot), np.median(frm), np.mean(frm), np.mean(chk), np.mean(rej)))


if __name__ == "__main__":
    main()
