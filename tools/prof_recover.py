"""Cost of vido_hamming_match_window and of Verify.Recover (profiles/r15/hamming_window.txt).

    rocprofv3 --kernel-trace -d DIR -o op --output-format csv -- python tools/prof_recover.py --op     # 50 launches per op and size, device-pointer form
    python tools/prof_recover.py --summarize DIR                                                       # median kernel time per launch from the trace
    VIDO_CALL_PROF=1 python tools/prof_recover.py --clip [--frames 12]                                 # the tracker on the corrupted clip: verify-only against recover

--op: queries and train entries as the tracker has them (positions on a 640 x 480 frame, levels 0 .. 7, radius 24, level_tol 1, max_dist 40, unique) at 1200 x 2000 and
3000 x 2500, and vido_hamming_match (the global 1-NN; csrc/hamming.hip) at the same sizes.  --clip: the clip and the corruption of tests/test_verify_recover_gpu.py;
the facade's timed_call table (printed at exit) holds hamming_match_window beside orb_describe_points."""
import argparse
import csv
import glob
import os
import sys
import tempfile
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((1200, 2000), (3000, 2500))
LAUNCHES = 50
WRONG = (16.0, -12.0); REGION_Y = 264; START = 1


def op():
    import torch
    import vido_slam_amd as V
    ctx = V.Context(width=640, height=480, max_batch=1)
    r = np.random.default_rng(0)
    for nq, nt in SIZES:
        mk = lambda n: (r.integers(0, 256, (n, 32), dtype=np.uint8), (r.random((n, 2)) * np.array([640, 480])).astype(np.float32), r.integers(0, 8, n).astype(np.int32))
        q = [torch.from_numpy(a).cuda() for a in mk(nq)]; t = [torch.from_numpy(a).cuda() for a in mk(nt)]
        out = [torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(4)]; st = torch.empty(5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            ctx.hamming_match_window_device(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), nq, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), nt, 24.0, 1, 40, None, True,
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), st.data_ptr())
        ctx.synchronize()
        print("window %d x %d: status counts %s" % (nq, nt, st.cpu().tolist()))
        for _ in range(LAUNCHES):
            ctx.hamming_match_device(q[0].data_ptr(), nq, t[0].data_ptr(), nt, out[0].data_ptr(), out[1].data_ptr())
        ctx.synchronize()
    ctx.close()


def summarize(d):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    by = {}
    for x in rows:
        name = x["Kernel_Name"].split("(")[0]
        if name.startswith("k_ham"):
            by.setdefault(name, []).append(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]))
    print("median kernel time per launch, us (%d launches per op and size; sizes in launch order: %s)" % (LAUNCHES, ", ".join("%d x %d" % s for s in SIZES)))
    tot = {}
    for name, v in by.items():
        per = [v[i * LAUNCHES:(i + 1) * LAUNCHES] for i in range(len(v) // LAUNCHES)]
        print("  %-18s " % name + "  ".join("%7.2f" % (np.median(c) / 1e3) for c in per))
        tot[name] = [np.median(c) / 1e3 for c in per]
    win = [k for k in tot if k.startswith("k_hamwin")]; old = [k for k in tot if not k.startswith("k_hamwin")]
    for label, names in (("vido_hamming_match_window (sum of its kernels)", win), ("vido_hamming_match (sum of its kernels)", old)):
        if names:
            print("  %-48s " % label + "  ".join("%7.2f" % sum(tot[k][i] for k in names) for i in range(len(tot[names[0]]))))


def settings(path, scene, extra):
    fx, fy, cx, cy = scene.K
    with open(path, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (scene.w, scene.h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: 387.57\nCamera.fps: 10.0\nCamera.RGB: 0\nChooseData: 1\nDepthMapFactor: 1.0\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n")
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n" + extra)
    return path


def clip(n):
    import vido_slam_amd as V
    from vido_slam_amd.system import System
    scene = V.synth.Scene3D(n_frames=n, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = []
    for k in range(n):
        g, d, f, m = scene.frame(k)
        if k >= START:
            f = f.copy(); sel = (m == 0); sel[REGION_Y:, :] = False; f[sel, 0] += WRONG[0]; f[sel, 1] += WRONG[1]
        frames.append((g, d, f, m))
    ver = "Verify.Descriptor: 1\n"; rec = ver + "Verify.Recover: 1\n"
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("verify ", ver), ("recover", rec), ("verify ", ver), ("recover", rec)):
            slam = System(); slam.Init(settings(os.path.join(tmp, "s.yaml"), scene, extra), System.RGBD)
            tot, frm, tried, got, keep = [], [], [], [], []
            for k, (g, d, f, m) in enumerate(frames):
                arrs = (g, np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)); keep.append(arrs)
                slam.TrackRGBD(*arrs, None, None, float(k), None, n)
                st = slam.stats(); a, b = slam.recover_stats()
                if k >= 3:
                    tot.append(st["ms_total"]); frm.append(st["ms_frame"]); tried.append(a); got.append(b)
            slam.close()
            print("%s frames 3..%d: ms_total median %.3f mean %.3f | ms_frame median %.3f mean %.3f | searched per frame %.0f, re-found %.0f" % (
                name, n - 1, np.median(tot), np.mean(tot), np.median(frm), np.mean(frm), np.mean(tried), np.mean(got)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", action="store_true"); ap.add_argument("--clip", action="store_true"); ap.add_argument("--summarize"); ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    if a.op:
        op()
    if a.summarize:
        summarize(a.summarize)
    if a.clip:
        clip(a.frames)
