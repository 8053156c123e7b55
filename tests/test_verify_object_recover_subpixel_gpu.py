"""GPU: Verify.ObjectRecoverSubpixel — the object points Verify.ObjectRecover re-finds on a whole pixel are aligned to 1/256 px against the patch they carry
(vido_orb_patch_refine, one call per frame, between the search and the gather); a refined point goes to re-found pixel + q8 / 256 + the fraction of its last position.

The clip is the corrupted-flow clip of tests/test_verify_object_recover_gpu.py (same scene, same corruption, same settings), rebuilt here.  The defaults (6 iterations,
window 1.5 px, min_eig 0) and the ratio the tracker is held to come from the CPU measurement kept in profiles/r19/patch_refine_cpu.txt (tools/measure_patch_refine.py,
numpy only, same renderer), line RATIO: the median distance to the true sub-pixel correspondence falls to TOOL_RATIO = 0.2845 of the whole pixel's.

The margin is built as that test builds its own, without the code under test: the numpy statement refines the points the RECOVER-ONLY run moved (centres and reference
patches from that run's read-back, references checked against what numpy cuts from the rendered previous frame), which gives the ratio this clip's population allows.
margin = max(0, that ratio - TOOL_RATIO) + the 3-sigma width of the two medians, taken in ranks (a median of n values lies between the values of rank n / 2 -+ 1.5 sqrt(n)):
the statement's upper rank over the recover-only run's lower rank, less the ratio of the medians.  profiles/r19/verify_object_recover_subpixel_gpu.txt keeps a run."""
import os
import numpy as np
import pytest

from refimpl import patch_points_np as PP
from refimpl import patch_refine_np as R

pytestmark = pytest.mark.gpu

ITERS, MAX_SHIFT_Q8, MIN_EIG = 6, 384, 0               # the defaults: profiles/r19/patch_refine_cpu.txt
TOOL_RATIO = 0.2845
WRONG = (0.0, 8.0)
START = 3
N = 10
TRUE_MOTION = np.array([0.25, 0.0, 0.05])
CLEAN_BOUND = 0.05                                     # the clean clip's bound of tests/test_verify_object_patch_gpu.py
VERIFY = "Verify.ObjectPatch: 1\n"
RECOVER = VERIFY + "Verify.ObjectRecover: 1\n"
SUBPIXEL = RECOVER + "Verify.ObjectRecoverSubpixel: 1\n"


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
    out = dict(poses=[], errs=[], stats=[], ostats=[], vp=[], rstats=[], rp=[], fstats=[], fp=[])
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
            out["fstats"].append(slam.object_refine_stats()); out["fp"].append(slam.object_refine_points())
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
    tmp = tmp_path_factory.mktemp("objsubpixel")
    scene = vido.synth.Scene3D(n_frames=N, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = [scene.frame(k) for k in range(N)]
    R_ = dict(scene=scene, frames=frames, blur=[oracle.gaussian_blur7(f[0]) for f in frames])
    R_["verify"] = _track(tmp, scene, frames, "verify", VERIFY)
    R_["alone"] = _track(tmp, scene, frames, "alone", VERIFY + "Verify.ObjectRecoverSubpixel: 1\nVerify.ObjectRecoverSubpixelIters: 3\n")      # without Verify.ObjectRecover the key is off
    R_["recover"] = _track(tmp, scene, frames, "recover", RECOVER)
    R_["zero"] = _track(tmp, scene, frames, "zero", RECOVER + "Verify.ObjectRecoverSubpixel: 0\nVerify.ObjectRecoverSubpixelIters: 2\nVerify.ObjectRecoverSubpixelMaxShift: 0.5\nVerify.ObjectRecoverSubpixelMinEig: 1000\n")
    R_["subpixel"] = _track(tmp, scene, frames, "subpixel", SUBPIXEL)
    return R_


def _refs(runs, vp, k):
    """reference patches numpy cuts from the previous frame at the previous positions, rounded as the tracker rounds them"""
    prev = np.rint(vp["prev_xy"]).astype(np.int32)
    return PP.take([runs["blur"][k - 1]], np.concatenate([prev, np.zeros((len(prev), 1), np.int32)], 1))


def _displaced(runs, vp, k):
    sel = _half(runs["frames"][k - 1][3]); p = np.rint(vp["prev_xy"]).astype(int)
    ok = (p[:, 0] >= 0) & (p[:, 0] < sel.shape[1]) & (p[:, 1] >= 0) & (p[:, 1] < sel.shape[0])
    out = np.zeros(len(p), bool); out[ok] = sel[p[ok, 1], p[ok, 0]]
    return out


def _truth(runs, vp, k):
    """the true sub-pixel correspondence of every verified point: its last position plus the RENDERED flow of frame k - 1 there (bilinear between pixels)"""
    p = vp["prev_xy"].astype(np.float64); flow = runs["frames"][k - 1][2].astype(np.float64); h, w = flow.shape[:2]
    x = np.clip(p[:, 0], 0, w - 1.001); y = np.clip(p[:, 1], 0, h - 1.001)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int); ax, ay = (x - x0)[:, None], (y - y0)[:, None]
    f = (1 - ay) * ((1 - ax) * flow[y0, x0] + ax * flow[y0, x0 + 1]) + ay * ((1 - ax) * flow[y0 + 1, x0] + ax * flow[y0 + 1, x0 + 1])
    return p + f


def _p_prime(centre, q8, prev_xy):
    """re-found pixel + q8 / 256 + (last position - lrintf(last position)), in double, rounded once to float"""
    prev = prev_xy.astype(np.float64)
    return (centre.astype(np.float64) + q8.astype(np.float64) / 256.0 + (prev - np.rint(prev_xy).astype(np.float64))).astype(np.float32)


def _same_run(A, B, tag):
    for k in range(N):
        assert np.array_equal(A["poses"][k], B["poses"][k]), (tag, k)
        assert A["stats"][k] == B["stats"][k] and A["ostats"][k] == B["ostats"][k] and A["rstats"][k] == B["rstats"][k], (tag, k)
        assert all(np.array_equal(A["vp"][k][key], B["vp"][k][key]) for key in A["vp"][k]), (tag, k)
        assert all(np.array_equal(A["rp"][k][key], B["rp"][k][key]) for key in A["rp"][k]), (tag, k)
    assert np.array_equal(A["motions"], B["motions"]), tag


def test_key_absent_zero_or_without_object_recover_changes_nothing(runs):
    """Verify.ObjectRecoverSubpixel: 0 with the three other keys set == the recover run, exactly: poses, stats, counts, both read-backs, saved object motions;
    Verify.ObjectRecoverSubpixel: 1 without Verify.ObjectRecover == the verification-only run.  The refine stats read 0 and the read-back is empty."""
    _same_run(runs["recover"], runs["zero"], "zero")
    _same_run(runs["verify"], runs["alone"], "alone")
    for name in ("verify", "alone", "recover", "zero"):
        assert all(s == (0, 0) for s in runs[name]["fstats"]) and all(len(v["status"]) == 0 for v in runs[name]["fp"]), name
    assert sum(s[1] for s in runs["recover"]["rstats"][START + 1:]) > 300


def test_read_back_recomputes_to_the_statement_and_the_points_hold_p_prime(runs):
    """Mechanics: status, q8 and cost of every point the search found are the numpy statement's at the read-back's own centres (xyl + dxy) and references (checked against
    what numpy cuts from the previous frame); a point the search did not find is not sent; a refined point that the gather accepts sits at p', its flow is p' minus the
    last position, both to float equality; an unrefined one keeps the whole pixel."""
    run = runs["subpixel"]; n_sent = n_refined = n_moved_sub = 0; seen = set()
    assert len(run["fp"][0]["status"]) == 0 and run["fstats"][0] == (0, 0)
    for k in range(1, N):
        vp, rp, fp = run["vp"][k], run["rp"][k], run["fp"][k]; n = len(vp["status"])
        assert n > 300 and all(len(fp[key]) == n for key in fp) and fp["cost"].dtype == np.int64
        ref, ok = _refs(runs, vp, k)
        assert np.array_equal(vp["ref_patch"], ref)
        found = rp["status"] == 0
        assert np.all(fp["status"][~found] == -2) and not fp["q8"][~found].any() and not fp["cost"][~found].any()
        centre = vp["xyl"][:, :2] + rp["dxy"]
        xyl = np.concatenate([centre, np.zeros((n, 1), np.int32)], 1).astype(np.int32)
        want = R.patch_refine([runs["blur"][k]], xyl[found], ref[found], ITERS, MAX_SHIFT_Q8, MIN_EIG)
        assert np.array_equal(fp["q8"][found], want[0]) and np.array_equal(fp["cost"][found], want[1]) and np.array_equal(fp["status"][found], want[3]), k
        refined = fp["status"] == 0
        assert run["fstats"][k] == (int(found.sum()), int(refined.sum()))
        moved = found & (rp["after"][:, 3] > 0)
        pp = np.where(refined[:, None], _p_prime(centre, fp["q8"], vp["prev_xy"]), centre.astype(np.float32))
        assert np.array_equal(rp["after"][moved, :2], pp[moved]) and np.array_equal(rp["after"][moved, 2:4], rp["gather"][moved])
        assert np.array_equal(rp["after"][moved, 4:6], pp[moved] - vp["prev_xy"][moved]) and np.all(rp["gather"][moved, 0] > 0)
        rej = vp["status"] == 1
        assert np.all(rp["after"][rej & ~moved, 3] == 0) and run["rstats"][k] == (int(rej.sum()), int(moved.sum()))
        n_sent += int(found.sum()); n_refined += int(refined.sum()); n_moved_sub += int((moved & refined & (fp["q8"] != 0).any(1)).sum()); seen |= set(fp["status"][found].tolist())
    print("sent %d, refined %d, moved off the whole pixel and accepted %d, statuses %s" % (n_sent, n_refined, n_moved_sub, sorted(seen)))
    assert n_sent > 300 and n_refined > 0.5 * n_sent and n_moved_sub > 100


def _rank_bounds(v):
    """(lower, median, upper): the values of rank n / 2 -+ 1.5 sqrt(n), the 3-sigma range of a median in ranks"""
    v = np.sort(v); n = len(v); d = 1.5 * np.sqrt(n)
    return v[max(int(np.floor(n / 2.0 - d)), 0)], float(np.median(v)), v[min(int(np.ceil(n / 2.0 + d)), n - 1)]


def test_refined_points_are_nearer_the_true_correspondence(runs):
    """Accuracy and the motion error of the three runs (profiles/r19/verify_object_recover_subpixel_gpu.txt)."""
    sub, rec, ver = runs["subpixel"], runs["recover"], runs["verify"]
    d_sub, d_rec, d_np = [], [], []; lines = []
    for k in range(START + 1, N):
        for run, dist in ((rec, d_rec), (sub, d_sub)):
            vp, rp = run["vp"][k], run["rp"][k]
            moved = _displaced(runs, vp, k) & (rp["status"] == 0) & (rp["after"][:, 3] > 0)
            dist.append(np.hypot(*(rp["after"][moved, :2].astype(np.float64) - _truth(runs, vp, k)[moved]).T))
        # the numpy statement at the points the recover-only run moved
        vp, rp = rec["vp"][k], rec["rp"][k]
        moved = _displaced(runs, vp, k) & (rp["status"] == 0) & (rp["after"][:, 3] > 0)
        ref, _ = _refs(runs, vp, k); centre = vp["xyl"][:, :2] + rp["dxy"]
        xyl = np.concatenate([centre, np.zeros((len(centre), 1), np.int32)], 1).astype(np.int32)
        w = R.patch_refine([runs["blur"][k]], xyl[moved], ref[moved], ITERS, MAX_SHIFT_Q8, MIN_EIG)
        pp = np.where((w[3] == 0)[:, None], _p_prime(centre[moved], w[0], vp["prev_xy"][moved]), centre[moved].astype(np.float32))
        d_np.append(np.hypot(*(pp.astype(np.float64) - _truth(runs, vp, k)[moved]).T))
        lines.append("frame %d: moved points of the displaced half: recover-only %d (median %.4f px), statement there %.4f px (refined %d), subpixel run %d (median %.4f px); sent / refined %s" % (
            k, len(d_rec[-1]), np.median(d_rec[-1]), np.median(d_np[-1]), int((w[3] == 0).sum()), len(d_sub[-1]), np.median(d_sub[-1]), sub["fstats"][k]))
    d_sub, d_rec, d_np = np.concatenate(d_sub), np.concatenate(d_rec), np.concatenate(d_np)
    lo_rec, m_rec, _ = _rank_bounds(d_rec); _, m_np, hi_np = _rank_bounds(d_np); m_sub = float(np.median(d_sub))
    ratio_np = m_np / m_rec
    margin = max(0.0, ratio_np - TOOL_RATIO) + (hi_np / lo_rec - ratio_np)
    e_sub, e_rec, e_ver = _motion_error(sub, START), _motion_error(rec, START), _motion_error(ver, START)
    print("\n".join(lines))
    print("distance to the true sub-pixel correspondence, moved points of the displaced half, frames %d .. %d:" % (START + 1, N - 1))
    print("  recover-only run  n %d  median %.4f  p90 %.4f px" % (len(d_rec), m_rec, np.percentile(d_rec, 90)))
    print("  statement there   n %d  median %.4f  p90 %.4f px   ratio %.4f (tool %.4f)" % (len(d_np), m_np, np.percentile(d_np, 90), ratio_np, TOOL_RATIO))
    print("  subpixel run      n %d  median %.4f  p90 %.4f px   ratio %.4f   bar %.4f = tool %.4f + margin %.4f" % (
        len(d_sub), m_sub, np.percentile(d_sub, 90), m_sub / m_rec, TOOL_RATIO + margin, TOOL_RATIO, margin))
    print("object motion error (mean, motions from frame %d on): subpixel %.5f  recover alone %.5f  verification alone %.5f" % (START, e_sub, e_rec, e_ver))
    for name, run in (("subpixel", sub), ("recover alone", rec), ("verification alone", ver)):
        print("object motion error per motion, %s:" % name, " ".join("%d: %.5f" % (int(r[0]), np.linalg.norm(r[2:14].reshape(3, 4)[:, 3] - TRUE_MOTION)) for r in run["motions"]))
    print("camera error subpixel:", ["%.5f" % e for e in sub["errs"]])
    print("sent / refined per frame:", sub["fstats"], " tried / recovered per frame:", sub["rstats"])
    assert len(d_rec) > 300 and len(d_sub) > 300
    assert m_sub < m_rec                                                             # nearer than the whole pixel
    assert m_sub <= (TOOL_RATIO + margin) * m_rec                                    # and by the tool's ratio, within what this clip's population allows
    assert e_sub < CLEAN_BOUND and max(sub["errs"]) < CLEAN_BOUND
