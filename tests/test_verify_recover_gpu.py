"""GPU: Verify.Recover — the static points that Verify.Descriptor has just rejected are searched among the frame's own static keypoints (vido_hamming_match_window, one
call per frame, unique = 1) and a re-found point moves onto its keypoint instead of being dropped.  Clip and corruption are those of tests/test_verify_flow_gpu.py (the
helpers are copies): from frame START on the rendered flow of the far wall carries one common wrong displacement.

The settings and the two shares of the last test come from the CPU measurement kept in profiles/r15/descriptor_recover.txt (tools/measure_descriptor_recover.py, oracle
only, same renderer, made before any GPU run; seeds of all ages): the selected setting re-finds TOOL_CORRECT of the rejected points at (16, -12) within 1.5 * scale[level] px of the true
position and puts TOOL_WRONG elsewhere; the test allows 5 points of percentage either way, the margin tests/test_verify_flow_gpu.py gives the RANSAC draws."""
import os
import numpy as np
import pytest

from refimpl.hamming_window_np import match_window

pytestmark = pytest.mark.gpu

MAX_HAMMING = 70
WRONG = (16.0, -12.0)
REGION_Y = 264
START = 1
EDGE = 19
POPCNT = np.array([bin(i).count("1") for i in range(256)], np.int32)
RADIUS, LEVEL_TOL, RECOVER_MAX_HAMMING, RATIO = 32.0, 1, 50, None        # the defaults (profiles/r15/descriptor_recover.txt), written out so that the test states them
TOOL_CORRECT, TOOL_WRONG = 0.268, 0.048                                       # at (16, -12), seeds of all ages
RECOVER = "Verify.Descriptor: 1\nVerify.MaxHamming: %d\nVerify.Recover: 1\n" % MAX_HAMMING


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


@pytest.fixture(scope="module")
def clip(vido):
    n = 12
    scene = vido.synth.Scene3D(n_frames=n, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    return scene, [scene.frame(k) for k in range(n)]


def _corrupt(flow, mask):
    f = flow.copy()
    sel = (mask == 0); sel[REGION_Y:, :] = False
    f[sel, 0] += WRONG[0]; f[sel, 1] += WRONG[1]
    return f


def _track(vido, settings, scene, frames, n, corrupt_from=None, per_frame=None):
    """Poses, errors and stats of the first n frames; per_frame(k, slam, inputs) is called after every frame with the arrays the tracker was given."""
    from vido_slam_amd.system import System
    slam = System(); slam.Init(settings, System.RGBD)
    poses, errs, stats, keep = [], [], [], []
    try:
        for k in range(n):
            g, d, f, m = frames[k]
            if corrupt_from is not None and k >= corrupt_from:
                f = _corrupt(f, m)
            d = np.ascontiguousarray(d, np.float32).copy(); f = np.ascontiguousarray(f, np.float32); m = np.ascontiguousarray(m, np.int32)
            T = slam.TrackRGBD(g, d, f, m, None, None, float(k), None, n)
            keep.append((g, d, f, m))
            E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
            poses.append(T.copy()); errs.append(float(np.linalg.norm(E[:3, 3])))
            st = slam.stats(); stats.append({key: v for key, v in st.items() if not key.startswith("ms_")})
            stats[-1]["verify"] = slam.verify_stats(); stats[-1]["recover"] = slam.recover_stats()
            if per_frame:
                per_frame(k, slam, (g, d, f, m))
    finally:
        slam.close()
    return poses, errs, stats


def _cpu_dist(oracle, p, levels, blurred, xyl, seed):
    out = np.full(len(xyl), -1, np.int32)
    for i, (x, y, l) in enumerate(xyl):
        if l < 0:
            continue
        h, w = levels[l].shape
        if not (EDGE <= x < w - EDGE and EDGE <= y < h - EDGE):
            continue
        d = oracle.brief(blurred[l], x, y, oracle.ic_angle(levels[l], x, y, p))
        out[i] = POPCNT[d ^ seed[i]].sum()
    return out


def test_option_off_is_inert(tmp_path, vido, clip):
    """Verify.Recover: 0 (with its other keys set) == the key absent, exactly: poses, counts, stats over 12 frames of the corrupted clip; and without Verify.Descriptor
    the key does nothing either."""
    scene, frames = clip
    a = _track(vido, _settings(tmp_path, scene, "plain.yaml", "Verify.Descriptor: 1\nVerify.MaxHamming: %d\n" % MAX_HAMMING), scene, frames, 12, corrupt_from=START)
    b = _track(vido, _settings(tmp_path, scene, "off.yaml", "Verify.Descriptor: 1\nVerify.MaxHamming: %d\nVerify.Recover: 0\nVerify.RecoverRadius: 3\nVerify.RecoverMaxHamming: 200\n" % MAX_HAMMING),
               scene, frames, 12, corrupt_from=START)
    rejected = 0
    for k in range(12):
        assert np.array_equal(a[0][k], b[0][k]), k
        assert a[2][k] == b[2][k], (k, a[2][k], b[2][k])
        assert a[2][k]["recover"] == (0, 0)
        rejected += a[2][k]["verify"][1]
    assert rejected > 3000                                                    # there was something to recover
    c = _track(vido, _settings(tmp_path, scene, "noverify.yaml"), scene, frames, 4, corrupt_from=START)
    d = _track(vido, _settings(tmp_path, scene, "alone.yaml", "Verify.Recover: 1\n"), scene, frames, 4, corrupt_from=START)
    for k in range(4):
        assert np.array_equal(c[0][k], d[0][k]) and c[2][k] == d[2][k] and d[2][k]["recover"] == (0, 0) and d[2][k]["verify"] == (0, 0)


def test_verdicts_equal_the_statement(tmp_path, vido, oracle, clip):
    """Frames 1 .. 5 of the corrupted clip.  The searched points are exactly the points the oracle's distance rejects; the train list read back is the frame's static
    candidate list (the oracle's keypoints through the oracle's static filter, on the maps the tracker was given); the numpy statement on those queries and that list
    reproduces status, index and both distances of every point; a re-found point sits on its keypoint with the keypoint's depth and the last frame's flow
    keypoint - last position (one fp32 subtraction per component), every other point is where it was; the counters count the same."""
    scene, frames = clip
    p = oracle.orb_params()
    seen = {"tried": 0, "recovered": 0, "status": set()}

    def check(k, slam, inputs):
        g, d, f, m = inputs
        vp = slam.verify_points(); rp = slam.recover_points()
        if k == 0:
            assert len(rp["status"]) == 0 and len(rp["train_xy"]) == 0 and slam.recover_stats() == (0, 0)
            return
        n = len(vp["dist"]); assert n > 300 and len(rp["status"]) == n
        levels = oracle.orb_pyramid(p, g); blurred = [oracle.gaussian_blur7(l) for l in levels]
        ref = _cpu_dist(oracle, p, levels, blurred, vp["xyl"], vp["seed_desc"])
        tried = ref > MAX_HAMMING
        assert np.array_equal(rp["status"] >= 0, tried)
        # the train list: this frame's keypoints that pass the static filter
        kps, desc, _ = oracle.orb_extract(p, g)
        sidx, _, _, sdep = oracle.static_candidates(kps, d, f, m, 40.0)
        assert np.array_equal(rp["train_xy"], np.stack([kps["x"][sidx], kps["y"][sidx]], 1)) and np.array_equal(rp["train_level"], kps["octave"][sidx])
        assert np.array_equal(rp["train_desc"], desc[sidx]) and np.array_equal(rp["train_depth"], sdep)
        q = np.flatnonzero(tried)
        idx, dist, dist2, status, stats = match_window(vp["seed_desc"][q], vp["xy"][q], vp["xyl"][q, 2], rp["train_desc"], rp["train_xy"], rp["train_level"],
                                                       RADIUS, LEVEL_TOL, RECOVER_MAX_HAMMING, RATIO, True)
        for name, want in (("status", status), ("idx", idx), ("dist", dist), ("dist2", dist2)):
            assert np.array_equal(rp[name][q], want), (k, name)
            assert (rp[name][~tried] == -1).all(), (k, name)
        rec = np.zeros(n, bool); rec[q] = status == 0
        j = rp["idx"][rec]
        assert len(set(j.tolist())) == len(j)                                  # one keypoint, one re-found point
        assert np.array_equal(rp["match_xy"][rec], rp["train_xy"][j]) and (rp["match_xy"][~rec] == -1).all()
        assert np.array_equal(rp["after"][rec, :2], rp["train_xy"][j]) and np.array_equal(rp["after"][rec, 2], rp["train_depth"][j])
        assert np.array_equal(rp["after"][rec, 3:5], rp["train_xy"][j] - vp["prev_xy"][rec])
        assert np.array_equal(rp["after"][~rec, :2], vp["xy"][~rec])
        assert np.array_equal(rp["after"][~rec, :2], (vp["prev_xy"][~rec].astype(np.float32) + rp["after"][~rec, 3:5]).astype(np.float32))
        assert np.array_equal(vp["rejected"], tried & ~rec)
        assert slam.recover_stats() == (int(tried.sum()), int(rec.sum())) and slam.verify_stats() == (int((ref >= 0).sum()), int((tried & ~rec).sum()))
        seen["tried"] += int(tried.sum()); seen["recovered"] += int(rec.sum()); seen["status"] |= set(status.tolist())

    _track(vido, _settings(tmp_path, scene, "on.yaml", RECOVER), scene, frames, 6, corrupt_from=START, per_frame=check)
    assert seen["tried"] > 1500 and seen["recovered"] > 300 and seen["status"] >= {0, 1, 2}


def test_recovery_keeps_the_points_and_the_pose(tmp_path, vido, oracle, clip):
    """12 frames, the far wall's flow displaced by WRONG from frame START on.  Of the wall's points that the verification rejects, the share re-found within
    1.5 * scale[level] px of the true correspondence (checked position - WRONG = last position + the uncorrupted flow) is at least TOOL_CORRECT - 0.05 and the share
    re-found elsewhere at most TOOL_WRONG + 0.05; the translation error with recovery is below the option-off tracker's on every corrupted frame and below 0.1 m (the line
    tests/test_verify_flow_gpu.py draws for "follows the wall") on every frame.  The error series and the number of static points that enter the pose are printed for the
    verify-only and the recover run (profiles/r15/verify_recover_gpu.txt keeps a run).

    Measured (MI355X, profiles/r15/verify_recover_gpu.txt): 8 760 points searched, 0.582 re-found at the true correspondence (floor 0.218), 0.051 elsewhere (cap 0.098);
    translation error 0.0003 .. 0.0039 m with recovery, 0.0003 .. 0.0041 m with verification alone, 1.26 m per frame with neither."""
    scene, frames = clip
    n = 12
    p = oracle.orb_params(); scale = np.array([p.scale[l] for l in range(8)], np.float32)
    cnt = {"tried": 0, "correct": 0, "elsewhere": 0}
    enter = {"recover": [], "verify": []}

    def count(k, slam, inputs):
        vp = slam.verify_points(); rp = slam.recover_points()
        enter["recover"].append(len(vp["dist"]) - int(vp["rejected"].sum()))
        if k <= START:
            return
        px, py = vp["prev_xy"][:, 0], vp["prev_xy"][:, 1]
        ok = (px >= 0) & (px < scene.w) & (py >= 0) & (py < scene.h)
        pm = frames[k - 1][3]
        inside = np.zeros(len(px), bool)
        inside[ok] = (py[ok] < REGION_Y - 1.5) & (pm[py[ok].astype(int), px[ok].astype(int)] == 0)
        near = (np.abs(py - REGION_Y) <= 1.5) | ~ok                            # (which side of the boundary the tracker's flow lookup took is not the test's business)
        cor = inside & ~near & (rp["status"] >= 0)
        truth = vp["xy"] - np.array(WRONG, np.float32)
        rec = cor & (rp["status"] == 0)
        err = np.hypot(rp["match_xy"][:, 0] - truth[:, 0], rp["match_xy"][:, 1] - truth[:, 1])
        good = rec & (err <= 1.5 * scale[np.maximum(vp["xyl"][:, 2], 0)])
        cnt["tried"] += int(cor.sum()); cnt["correct"] += int(good.sum()); cnt["elsewhere"] += int((rec & ~good).sum())

    def count_verify(k, slam, inputs):
        vp = slam.verify_points()
        enter["verify"].append(len(vp["dist"]) - int(vp["rejected"].sum()))

    rec = _track(vido, _settings(tmp_path, scene, "rec.yaml", RECOVER), scene, frames, n, corrupt_from=START, per_frame=count)
    ver = _track(vido, _settings(tmp_path, scene, "ver.yaml", "Verify.Descriptor: 1\nVerify.MaxHamming: %d\n" % MAX_HAMMING), scene, frames, n, corrupt_from=START, per_frame=count_verify)
    off = _track(vido, _settings(tmp_path, scene, "off.yaml"), scene, frames, n, corrupt_from=START)
    share_correct = cnt["correct"] / max(cnt["tried"], 1); share_elsewhere = cnt["elsewhere"] / max(cnt["tried"], 1)
    print("translation error verify-only:", ["%.5f" % e for e in ver[1]])
    print("translation error    recover :", ["%.5f" % e for e in rec[1]])
    print("translation error  option off:", ["%.5f" % e for e in off[1]])
    print("static points entering the pose, verify-only:", enter["verify"])
    print("static points entering the pose,    recover :", enter["recover"])
    print("searched / re-found per frame (recover):", [s["recover"] for s in rec[2]])
    print("rejected wall points searched %d: re-found at the true correspondence %.3f (floor %.3f), elsewhere %.3f (cap %.3f)" % (
        cnt["tried"], share_correct, TOOL_CORRECT - 0.05, share_elsewhere, TOOL_WRONG + 0.05))
    assert cnt["tried"] > 3000
    assert off[1][START + 1] > 0.1                                              # the premise: without any option the tracker follows the wall
    for k in range(START + 1, n):
        assert rec[1][k] < off[1][k], (k, rec[1][k], off[1][k])
    for k in range(n):
        assert rec[1][k] < 0.1, (k, rec[1][k])
    assert share_correct >= TOOL_CORRECT - 0.05
    assert share_elsewhere <= TOOL_WRONG + 0.05
