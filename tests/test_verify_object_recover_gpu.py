"""GPU: Verify.ObjectRecover — the dense object points that Verify.ObjectPatch rejects are searched for in a window around the pixel that was verified
(vido_orb_patch_search, one call per frame); a found point moves to the re-found pixel if the frame's maps hold its own object there.

The clip is the corrupted-flow clip of tests/test_verify_object_patch_gpu.py, rebuilt here: from frame START on the flow over the right half of the object carries 8 px more
in y.  The defaults (radius 8, excl 2, gate 976 / 1024, peak test off) and the two shares the tracker is held to come from the CPU measurement kept in
profiles/r17/patch_recover.txt (tools/measure_patch_recover.py, numpy only, same renderer), row "displaced 8 px": TOOL_RIGHT_8PX = 0.8867 of the rejected textured points are
re-found within 1 px of the rounded true correspondence, TOOL_WRONG_8PX = 0.0614 are accepted on another pixel.

The margin is the construction of the patch-verification test.  The tool's population is every dense sample of 11 frames; the tracker's is the points its RANSAC and its
top-up left on THIS clip.  What that costs is measured without the code under test: the numpy statement searches at the positions the verification-only run rejected, with
reference patches numpy cuts from the previous frame the test rendered.  margin = max(0, tool share - that share) + 3 sqrt(p (1 - p) / n) for the right share, and
max(0, that share - tool share) + 3 sqrt(p (1 - p) / n) for the wrong share.  The right share counts the points the tracker really moved (found AND on their own object);
the wrong share counts every found point on another pixel, accepted or not: both the harder reading.  profiles/r17/verify_object_recover_gpu.txt keeps the figures of a run."""
import os
import numpy as np
import pytest

from refimpl import patch_points_np as PP
from refimpl import patch_search_np as R

pytestmark = pytest.mark.gpu

MIN_STD, MIN_Q10 = 6, 920
MIN_VAR = 4096 * MIN_STD * MIN_STD
RADIUS, EXCL, REC_Q10, REC_RATIO = 8, 2, 976, 0        # the defaults: profiles/r17/patch_recover.txt
TOOL_RIGHT_8PX = 0.8867
TOOL_WRONG_8PX = 0.0614
WRONG = (0.0, 8.0)
START = 3
N = 10
TRUE_MOTION = np.array([0.25, 0.0, 0.05])
CLEAN_BOUND = 0.05                                     # the clean clip's bound of tests/test_verify_object_patch_gpu.py
VERIFY = "Verify.ObjectPatch: 1\n"
RECOVER = "Verify.ObjectPatch: 1\nVerify.ObjectRecover: 1\n"


def _settings(tmp, scene, name, extra=""):
    fx, fy, cx, cy = scene.K
    p = os.path.join(str(tmp), name)
    with open(p, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (scene.w, scene.h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: 387.57\nCamera.fps: 10.0\nCamera.RGB: 0\nChooseData: 1\nDepthMapFactor: 1.0\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n")
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n")
        fh.write(extra)
    return p


def _half(mask):
    """the corrupted region: the object's pixels from the mask's median column on"""
    cols = np.flatnonzero((mask != 0).any(0))
    sel = mask != 0; sel[:, :int(np.median(cols))] = False
    return sel


def _track(tmp, scene, frames, name, extra):
    from vido_slam_amd.system import System
    slam = System(); slam.Init(_settings(tmp, scene, name + ".yaml", extra), System.RGBD)
    out = dict(poses=[], errs=[], stats=[], ostats=[], vp=[], rstats=[], rp=[])
    try:
        for k in range(N):
            g, d, f, m = frames[k]
            if k >= START:
                f = f.copy(); sel = _half(m); f[sel, 0] += WRONG[0]; f[sel, 1] += WRONG[1]
            d = np.ascontiguousarray(d, np.float32).copy(); f = np.ascontiguousarray(f, np.float32); m = np.ascontiguousarray(m, np.int32)
            T = slam.TrackRGBD(g, d, f, m, None, None, float(k), None, N)
            E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
            out["poses"].append(T.copy()); out["errs"].append(float(np.linalg.norm(E[:3, 3])))
            out["stats"].append({key: v for key, v in slam.stats().items() if not key.startswith("ms_")})
            out["ostats"].append(slam.object_verify_stats()); out["vp"].append(slam.object_verify_points())
            out["rstats"].append(slam.object_recover_stats()); out["rp"].append(slam.object_recover_points())
        prefix = os.path.join(str(tmp), name + "_")
        slam.SaveResultsIJRR2020(prefix)
        out["motions"] = np.loadtxt(prefix + "obj_mot_rgbd_new.txt", ndmin=2)
    finally:
        slam.close()
    return out


def _motion_error(run, first):
    rows = [r for r in run["motions"] if r[0] >= first]
    assert len(rows) >= N - first - 2, len(rows)
    return float(np.mean([np.linalg.norm(r[2:14].reshape(3, 4)[:, 3] - TRUE_MOTION) for r in rows]))


@pytest.fixture(scope="module")
def runs(vido, oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("objrecover")
    scene = vido.synth.Scene3D(n_frames=N, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = [scene.frame(k) for k in range(N)]
    R_ = dict(scene=scene, frames=frames, blur=[oracle.gaussian_blur7(f[0]) for f in frames])
    R_["off"] = _track(tmp, scene, frames, "off", "")
    R_["alone"] = _track(tmp, scene, frames, "alone", "Verify.ObjectRecover: 1\nVerify.ObjectRecoverRadius: 12\n")      # without Verify.ObjectPatch the key is off
    R_["verify"] = _track(tmp, scene, frames, "verify", VERIFY)
    R_["zero"] = _track(tmp, scene, frames, "zero", VERIFY + "Verify.ObjectRecover: 0\nVerify.ObjectRecoverRadius: 16\nVerify.ObjectRecoverMinZncc: 0.1\nVerify.ObjectRecoverExcl: 1\nVerify.ObjectRecoverPeakRatio: 0.5\n")
    R_["recover"] = _track(tmp, scene, frames, "recover", RECOVER)
    return R_


def _refs(runs, vp, k):
    """reference patches numpy cuts from the previous frame at the previous (integer) positions"""
    prev = np.rint(vp["prev_xy"]).astype(np.int32)
    return PP.take([runs["blur"][k - 1]], np.concatenate([prev, np.zeros((len(prev), 1), np.int32)], 1))


def _displaced(runs, vp, k):
    sel = _half(runs["frames"][k - 1][3]); p = np.rint(vp["prev_xy"]).astype(int)
    ok = (p[:, 0] >= 0) & (p[:, 0] < sel.shape[1]) & (p[:, 1] >= 0) & (p[:, 1] < sel.shape[0])
    out = np.zeros(len(p), bool); out[ok] = sel[p[ok, 1], p[ok, 0]]
    return out


def _truth(runs, vp, k):
    """the rounded true correspondence of every verified point: its last (integer) position plus the RENDERED flow of frame k - 1 there"""
    p = np.rint(vp["prev_xy"]).astype(int); flow = runs["frames"][k - 1][2]; h, w = flow.shape[:2]
    px = np.clip(p[:, 0], 0, w - 1); py = np.clip(p[:, 1], 0, h - 1)
    return np.rint(p + flow[py, px].astype(np.float64)).astype(int)


def _margin(tool, share, n, upper=False):
    return max(0.0, (share - tool) if upper else (tool - share)) + 3.0 * np.sqrt(tool * (1.0 - tool) / max(n, 1))


def test_key_absent_zero_or_without_object_patch_changes_nothing(runs):
    """(a) Verify.ObjectRecover: 0 with the four other keys set == the verification-only run, exactly: poses, stats, verification counts and read-back, saved object
    motions; Verify.ObjectRecover: 1 without Verify.ObjectPatch == the run with neither key.  The recover stats read 0 and the read-back is empty."""
    for a, b in (("verify", "zero"), ("off", "alone")):
        A, B = runs[a], runs[b]
        for k in range(N):
            assert np.array_equal(A["poses"][k], B["poses"][k]), (b, k)
            assert A["stats"][k] == B["stats"][k] and A["ostats"][k] == B["ostats"][k], (b, k)
            assert all(np.array_equal(A["vp"][k][key], B["vp"][k][key]) for key in A["vp"][k]), (b, k)
        assert np.array_equal(A["motions"], B["motions"]), b
    for name in ("off", "alone", "verify", "zero"):
        assert all(s == (0, 0) for s in runs[name]["rstats"]) and all(len(v["status"]) == 0 for v in runs[name]["rp"]), name
    assert sum(s[1] for s in runs["verify"]["ostats"][START + 1:]) > 300


def test_read_back_recomputes_to_the_statement(runs):
    """(b) status, dxy, sums and second of every searched point are the numpy statement's at the read-back's own positions, with reference patches numpy cuts from the
    previous frame; a point the verification did not reject is not searched; what the step left behind follows from the call and the gather."""
    run = runs["recover"]; n_tried = n_acc = 0
    assert len(run["rp"][0]["status"]) == 0 and run["rstats"][0] == (0, 0)
    for k in range(1, N):
        vp, rp = run["vp"][k], run["rp"][k]; n = len(vp["status"])
        assert n > 300 and all(len(rp[key]) == n for key in rp)
        ref, ok = _refs(runs, vp, k)
        assert np.array_equal(vp["ref_patch"], ref)
        rej = vp["status"] == 1
        assert np.all(rp["status"][~rej] == -2) and not rp["dxy"][~rej].any() and not rp["sums"][~rej].any() and not rp["second"][~rej].any()
        want = R.patch_search([runs["blur"][k]], vp["xyl"][rej], ref[rej], RADIUS, EXCL, MIN_VAR, REC_Q10, REC_RATIO)
        for key, w_ in zip(("dxy", "sums", "second", "status"), want[:4]):
            assert np.array_equal(rp[key][rej], w_), (k, key)
        found = rp["status"] == 0
        assert np.all(rp["gather"][~found] == -1)
        moved = found & (rp["after"][:, 3] > 0)
        p2 = (vp["xyl"][:, :2] + rp["dxy"]).astype(np.float32)
        assert np.array_equal(rp["after"][moved, :2], p2[moved]) and np.array_equal(rp["after"][moved, 2:4], rp["gather"][moved])
        assert np.array_equal(rp["after"][moved, 4:6], p2[moved] - vp["prev_xy"][moved]) and np.all(rp["gather"][moved, 0] > 0)
        assert np.all(rp["after"][rej & ~moved, 3] == 0)                      # still rejected: off its object
        assert run["rstats"][k] == (int(rej.sum()), int(moved.sum()))
        st = vp["status"]
        assert run["ostats"][k] == (int(((st == 0) | (st == 1)).sum()), int(rej.sum()) - int(moved.sum()), int((st == 2).sum()))
        n_tried += int(rej.sum()); n_acc += int(moved.sum())
    assert n_tried > 300 and n_acc > 100


def test_rejected_points_are_re_found_at_the_true_correspondence(runs):
    """(c), (d), (e)"""
    rec, ver, off = runs["recover"], runs["verify"], runs["off"]
    n = right = wrong = s_n = s_right = s_wrong = 0; lines = []
    for k in range(START + 1, N):
        vp, rp = rec["vp"][k], rec["rp"][k]
        pop = _displaced(runs, vp, k) & (vp["status"] == 1)
        truth = _truth(runs, vp, k); p2 = vp["xyl"][:, :2] + rp["dxy"]
        near = np.abs(p2 - truth).max(1) <= 1
        moved = (rp["status"] == 0) & (rp["after"][:, 3] > 0)
        n += int(pop.sum()); right += int((pop & moved & near).sum()); wrong += int((pop & (rp["status"] == 0) & ~near).sum())
        # the numpy statement at the positions the verification-only run rejected
        v = ver["vp"][k]; vpop = _displaced(runs, v, k) & (v["status"] == 1)
        ref, _ = _refs(runs, v, k)
        w = R.patch_search([runs["blur"][k]], v["xyl"][vpop], ref[vpop], RADIUS, EXCL, MIN_VAR, REC_Q10, REC_RATIO)
        vnear = np.abs(v["xyl"][vpop, :2] + w[0] - _truth(runs, v, k)[vpop]).max(1) <= 1
        s_n += int(vpop.sum()); s_right += int(((w[3] == 0) & vnear).sum()); s_wrong += int(((w[3] == 0) & ~vnear).sum())
        on_obj = int((rp["after"][:, 3] > 0).sum())
        lines.append("frame %d: carried %d, rejected %d, re-found and accepted %d; on their object after the step %d (verification alone: %d); verification-only run: carried %d, rejected %d" % (
            k, len(vp["status"]), rec["rstats"][k][0], rec["rstats"][k][1], on_obj, on_obj - rec["rstats"][k][1], len(v["status"]), ver["ostats"][k][1]))
        assert rec["rstats"][k][1] >= 1                                                  # (d) the same frame with verification alone has that many fewer points on the object
    share_r, share_w, s_r, s_w = right / n, wrong / n, s_right / s_n, s_wrong / s_n
    m_r = _margin(TOOL_RIGHT_8PX, s_r, s_n); m_w = _margin(TOOL_WRONG_8PX, s_w, s_n, upper=True)
    e_rec, e_ver, e_off = _motion_error(rec, START), _motion_error(ver, START), _motion_error(off, START)
    print("\n".join(lines))
    print("corrupted clip: rejected textured points on the displaced half %d; moved to within 1 px of the truth %.4f, found on another pixel %.4f" % (n, share_r, share_w))
    print("the statement at the verification-only run's rejected points: %d, right %.4f wrong %.4f; tool right %.4f wrong %.4f; margins %.4f %.4f; floor %.4f ceiling %.4f" % (
        s_n, s_r, s_w, TOOL_RIGHT_8PX, TOOL_WRONG_8PX, m_r, m_w, TOOL_RIGHT_8PX - m_r, TOOL_WRONG_8PX + m_w))
    print("object motion error (mean, motions from frame %d on): recover %.5f  verification only %.5f  off %.5f" % (START, e_rec, e_ver, e_off))
    for name, run in (("recover", rec), ("verification only", ver)):
        print("object motion error per motion, %s:" % name, " ".join("%d: %.5f" % (int(r[0]), np.linalg.norm(r[2:14].reshape(3, 4)[:, 3] - TRUE_MOTION)) for r in run["motions"]))
    print("camera error recover:", ["%.5f" % e for e in rec["errs"]])
    print("tried / recovered per frame:", rec["rstats"])
    assert n > 300 and s_n > 300
    assert share_r >= TOOL_RIGHT_8PX - m_r                                           # (c)
    assert share_w <= TOOL_WRONG_8PX + m_w
    assert sum(s[1] for s in rec["rstats"][START + 1:]) > 0.5 * sum(s[0] for s in rec["rstats"][START + 1:])      # (d) over the corrupted frames most of what was rejected is back
    assert e_rec < CLEAN_BOUND and max(rec["errs"]) < CLEAN_BOUND                    # (e)


def test_patches_stay_aligned_with_the_object_list(runs):
    """(f) Frame k's reference patches are frame k - 1's patch vector: one per object point frame k - 1 ended with, each the previous frame's blurred level 0 around the
    point's own (integer) position — through frames where points were moved by the search; keys, depth and labels of the read-back have the list's length."""
    run = runs["recover"]; moved_frames = 0
    for k in range(1, N):
        vp, rp = run["vp"][k], run["rp"][k]
        assert len(vp["status"]) == run["stats"][k - 1]["n_object_points"] == len(rp["status"]) == len(rp["after"])
        assert np.array_equal(vp["prev_xy"], np.rint(vp["prev_xy"]))
        ref, ok = _refs(runs, vp, k)
        assert ok.sum() > 300 and np.array_equal(vp["ref_patch"], ref)
        if k >= 2 and run["rstats"][k - 1][1] > 20:
            moved_frames += 1
    assert moved_frames >= 3
