"""MI355X: rectification inside the network nodes.  One module-scoped NetNodes(flow_source="dis", depth_source="stereo", detect_every=2, stereo_filter=True,
propagate_bf=235, rectify=dict(left=..., right=...)) over the rig of tests/test_stereo_rectify_cpu.py scaled to 640 x 480 (K_raw = (500, 500, 319.5, 239.5),
P = (470, 470, 319.5, 239.5), the KAIST coefficients, about 1 degree per camera): the constructor's refusals; rectify_frames equal to the numpy statement; infer()'s
disparity -1, stereo_status 5 and collision depth FLT_MAX outside rect_inside and the ops' own outputs inside; EndToEnd.push of RAW pairs leaves the rectified frames in
the ring slot; and the tracker on the 12-frame Scene3D clip of tests/test_stereo_pipeline_gpu.py seen through the raw rig (translation error <= 0.05 m on every frame,
the project's bar for a map source on this clip).  Nodes built without rectify are what the other pipeline test files build: their exact-equality tests are the check
that nothing changes there.  Each GPU step runs under limit().  profiles/r27/stereo_rectify_tracker_gpu.txt keeps the tracker's series of a run, beside the run on
the pair rendered directly in the rectified cameras (a report, not a bar)."""
import os

import numpy as np
import pytest
import torch

from refimpl import stereo_rectify_np as G
from refimpl import stereo_rectify_cases as CASES
from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

N_TRACK = 12
MAX_TRANSLATION_ERROR = 0.05
BASELINE = 0.5
W, H = 640, 480
P_RECT = (470.0, 470.0, 319.5, 239.5)
K_RAW = (500.0, 500.0, 319.5, 239.5)
BF = 235.0
PARAMS = dict(max_disp=64, p2=100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(3.4028234663852886e38)

CAL_L = dict(K=K_RAW, dist=CASES.KAIST_DIST, R=CASES.R_LEFT, P=P_RECT)
CAL_R = dict(K=K_RAW, dist=CASES.KAIST_DIST, R=CASES.R_RIGHT, P=P_RECT)


def _scene(vido, n=4):
    return vido.synth.Scene3D(n_frames=n, w=W, h=H, K=P_RECT, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))


def _raw_pair(scene, k):
    return scene.raw_stereo_frame(k, BASELINE, K_RAW, CASES.KAIST_DIST, CASES.R_LEFT, CASES.R_RIGHT)


@pytest.fixture(scope="module")
def maps():
    return [G.rectify_map(c["K"], c["dist"], c["R"], c["P"], (W, H), (W, H)) for c in (CAL_L, CAL_R)]


@pytest.fixture(scope="module")
def nodes(vido):
    from vido_slam_amd import pipeline
    with limit(600, "building NetNodes(rectify=...)"):
        n = pipeline.NetNodes(vido.Context(width=W, height=H, max_batch=1), H, W, flow_source="dis", depth_source="stereo", stereo_params=PARAMS, detect_every=2,
                              stereo_filter=True, propagate_bf=BF, rectify=dict(left=CAL_L, right=CAL_R))
        torch.cuda.synchronize()
    return n


def test_constructor_checks(vido):
    """Refused before anything is built: the context argument is None, so a check that came late would fail otherwise."""
    from vido_slam_amd import pipeline
    N = pipeline.NetNodes
    for kw in (dict(rectify=dict(left=CAL_L, right=CAL_R)),                                            # a right calibration without stereo depth
               dict(rectify=dict(left=CAL_L), depth_source="stereo"),                                  # stereo depth over raw frames needs both
               dict(rectify=dict(left=CAL_L, middle=CAL_R)), dict(rectify=dict(right=CAL_R), depth_source="stereo"), dict(rectify=[CAL_L]), dict(rectify=True),
               dict(rectify=dict(left=dict(CAL_L, k4=0.0))), dict(rectify=dict(left={k: v for k, v in CAL_L.items() if k != "R"})),
               dict(rectify=dict(left=dict(CAL_L, K=(500.0, 500.0, 319.5)))), dict(rectify=dict(left=dict(CAL_L, K=(0.0, 500.0, 319.5, 239.5)))),
               dict(rectify=dict(left=dict(CAL_L, R=np.full((3, 3), np.nan)))), dict(rectify=dict(left=dict(CAL_L, dist="none"))),
               dict(rectify=dict(left=CAL_L, raw_size=(8, 640))), dict(rectify=dict(left=CAL_L, raw_size=(480, 5000))), dict(rectify=dict(left=CAL_L, raw_size=640))):
        with pytest.raises(ValueError):
            N(None, H, W, **kw)
    assert N._check_rectify(None, "net", H, W) is None and N._check_rectify(None, "stereo", H, W) is None
    got = N._check_rectify(dict(left=dict(CAL_L, dist=CASES.KAIST_DIST[:4]), raw_size=(240, 320)), "net", H, W)
    assert got["right"] is None and got["raw_size"] == (240, 320) and got["left"]["dist"].tolist() == list(CASES.KAIST_DIST[:4]) + [0.0]


def test_rectify_frames_and_inside_masking(vido, nodes, maps):
    scene = _scene(vido)
    raw_l, raw_r = (vido.synth.gray_to_bgr(g) for g in _raw_pair(scene, 1))
    want_l, ins_l = G.rectify(raw_l, maps[0][0]); want_r, _ = G.rectify(raw_r, maps[1][0])
    assert nodes.rectify is not None and nodes.g_depth is not None, nodes.graph_error
    assert nodes.rect_inside.dtype == torch.bool and np.array_equal(nodes.rect_inside.cpu().numpy(), maps[0][1].astype(bool)) and np.array_equal(ins_l, maps[0][1])
    inside = maps[0][1].astype(bool)
    assert 0.85 <= inside.mean() < 1.0
    tl, tr = torch.as_tensor(raw_l, device="cuda"), torch.as_tensor(raw_r, device="cuda")
    with pytest.raises(ValueError):
        nodes.rectify_frames(tl)                                                       # two calibrations: the right frame is required
    with pytest.raises(ValueError):
        nodes.rectify_frames(tl[:100], tr)
    with limit(120, "rectify_frames, then infer() with the depth graph and eagerly"):
        rl, rr = nodes.rectify_frames(tl, tr)
        torch.cuda.synchronize()
        assert np.array_equal(rl.cpu().numpy(), want_l) and np.array_equal(rr.cpu().numpy(), want_r)
        ol, orr = torch.zeros_like(rl), torch.zeros_like(rr)
        got = nodes.rectify_frames(tl, tr, out_left=ol, out_right=orr)
        torch.cuda.synchronize()
        assert got[0] is ol and got[1] is orr and torch.equal(ol, rl) and torch.equal(orr, rr)
        ref = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
        _, q4, st, _ = ref.stereo_sgm(want_l, want_r, **PARAMS)
        disp, st2, plane, _ = ref.stereo_filter(q4, st, bf=BF)
        ref.close()
        for eager in (False, True):
            nodes._set_detect_every(2)
            if eager:
                g_depth, nodes.g_depth = nodes.g_depth, None
            try:
                flow, depth, mask, labels, evs = nodes.infer(rl, rl, right_bgr=rr)
                torch.cuda.synchronize()
            finally:
                if eager:
                    nodes.g_depth = g_depth
            d = depth.cpu().numpy(); s = nodes.stereo_status.cpu().numpy(); c = nodes._coll[nodes._coll_i].cpu().numpy()
            assert (d[~inside] == -1).all() and (s[~inside] == 5).all() and (c[~inside].view(np.uint32) == 0x7F7FFFFF).all(), eager
            assert np.array_equal(d[inside], disp[inside]) and np.array_equal(s[inside], st2[inside]) and c[inside].tobytes() == plane[inside].tobytes(), eager
            assert (s[inside] != 5).all() and (d[inside] > 0).mean() > 0.5
    print("outside the rectified view: %d pixels, of which the ops alone mark %d valid" % ((~inside).sum(), (st2[~inside] == 0).sum()))


def test_end_to_end_rectifies_raw_pairs_into_the_ring(vido, nodes, maps, tmp_path):
    from vido_slam_amd import pipeline
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    scene = _scene(vido, 5)
    frames = [scene.frame(k) for k in range(3)]
    raws = [_raw_pair(scene, k) for k in range(3)]
    want = [(G.rectify(vido.synth.gray_to_bgr(l_), maps[0][0])[0], G.rectify(vido.synth.gray_to_bgr(r_), maps[1][0])[0]) for l_, r_ in raws]
    inside = maps[0][1].astype(bool)
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    nodes._set_detect_every(2)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    try:
        with pytest.raises(ValueError):
            e2e.push(vido.synth.gray_to_bgr(raws[0][0]), None)                         # stereo nodes: a frame without its right view is refused
        with limit(180, "3 raw pairs through EndToEnd"):
            for k in range(3):
                g, d, f, m = frames[k]
                e2e.push(vido.synth.gray_to_bgr(raws[k][0]), (np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)),
                         right=vido.synth.gray_to_bgr(raws[k][1]))
            e2e.finish()
            torch.cuda.synchronize()
            left = [e2e.dev[k]["bgr"].cpu().numpy() for k in range(3)]; right = [e2e.dev[k]["right"].cpu().numpy() for k in range(3)]
            raw_parked = [e2e.dev[k]["raw"].cpu().numpy() for k in range(3)]
            depth = [e2e.dev[k]["depth"].cpu().numpy() for k in range(3)]
    finally:
        e2e.close(); slam.close()
    assert e2e.err is None and len(e2e.poses) == 3
    for k in range(3):
        assert np.array_equal(left[k], want[k][0]) and np.array_equal(right[k], want[k][1]), k
        assert np.array_equal(raw_parked[k], vido.synth.gray_to_bgr(raws[k][0])), k
        assert (depth[k][~inside] == -1).all() and (depth[k][inside] > 0).mean() > 0.5, k
    assert not np.array_equal(left[0], vido.synth.gray_to_bgr(raws[0][0]))


def _stereo_settings(tmp, scene, name):
    """The settings a rectified run needs: P's intrinsics, zero distortion, the KITTI ChooseData code (the depth image is a disparity), DepthMapFactor 1, bf = fx' * baseline"""
    fx, fy, cx, cy = scene.K
    p = os.path.join(str(tmp), name)
    with open(p, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (scene.w, scene.h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: %.1f\nCamera.fps: 10.0\nCamera.RGB: 0\nChooseData: 2\nDepthMapFactor: 1\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n" % (fx * BASELINE))
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n")
    return p


def test_tracker_on_the_rectified_rig(vido, maps, tmp_path):
    """The 12-frame Scene3D clip (one object, rendered flow and mask) seen through the raw rig: frame k's image is vido_rectify of the raw left frame, its depth the
    disparity vido_stereo_sgm finds on the rectified pair, -1 outside the rectified view, under settings with P's intrinsics, zero distortion and Camera.bf = 235.
    Condition: the camera's translation error is <= 0.05 m at every frame.  Beside it, as a report, the same clip on the pair rendered directly in the rectified cameras."""
    from test_verify_flow_gpu import _track
    scene = vido.synth.Scene3D(n_frames=N_TRACK + 2, w=W, h=H, K=P_RECT, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    assert scene.K[0] * BASELINE == BF
    inside = maps[0][1].astype(bool)
    ctx = vido.Context(width=W, height=H, max_batch=1)
    lines = []
    with limit(240, "12 raw pairs: render, rectify, match"):
        rect, direct, share, med = [], [], [], []
        for k in range(N_TRACK):
            g, depth, flow, mask = scene.frame(k)
            raw_l, raw_r = _raw_pair(scene, k)
            rl, rr, il, _ = ctx.rectify(raw_l, maps[0][0], raw_r, maps[1][0])
            assert np.array_equal(il, maps[0][1])
            disp = ctx.stereo_sgm(rl, rr, **PARAMS)[0]
            disp[~inside] = -1
            true = scene.K[0] * BASELINE / depth.astype(np.float64)
            ok = disp > 0
            share.append(float(ok.mean())); med.append(float(np.median(np.abs(disp[ok] - true[ok]))))
            rect.append((rl, disp, flow, mask))
            left, right, _, _ = scene.stereo_frame(k, BASELINE)
            direct.append((left, ctx.stereo_sgm(left, right, **PARAMS)[0], flow, mask))
        ctx.close()
    lines.append("rig: K_raw %s, P %s, KAIST coefficients, baseline %.1f m, bf %.0f; rect_inside share %.4f" % (K_RAW, P_RECT, BASELINE, BF, inside.mean()))
    lines.append("vido_stereo_sgm (max_disp 64, p2 100) on the rectified raw pair against Scene3D's disparity, per frame: share of all pixels valid "
                 + " ".join("%.3f" % s for s in share) + "; median |error| px of those " + " ".join("%.3f" % m for m in med))
    with limit(120, "12 frames, the pair rendered in the rectified cameras"):
        _, err_direct, _ = _track(vido, _stereo_settings(tmp_path, scene, "direct.yaml"), scene, direct, N_TRACK)
    with limit(120, "12 frames, the rectified raw pair"):
        _, err_rect, _ = _track(vido, _stereo_settings(tmp_path, scene, "rect.yaml"), scene, rect, N_TRACK)
    lines.append("translation error m, pair rendered in the rectified cameras (report): " + " ".join("%.4f" % e for e in err_direct))
    lines.append("translation error m, raw pair through vido_rectify:                   " + " ".join("%.4f" % e for e in err_rect))
    lines.append("condition: translation error <= %.2f m at every frame on the rectified raw pair: max %.4f m -> %s" % (
        MAX_TRANSLATION_ERROR, max(err_rect), "met" if max(err_rect) <= MAX_TRANSLATION_ERROR else "MISSED"))
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r27"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r27", "stereo_rectify_tracker_gpu.txt"), "w") as fh:
            fh.write("tests/test_stereo_rectify_pipeline_gpu.py::test_tracker_on_the_rectified_rig — Scene3D(seed 3, one object), 12 frames, 640 x 480, MI355X\n" + "\n".join(lines) + "\n")
    except OSError:
        pass                                                                          # (a read-only tree: the figures are printed above)
    assert min(share) > 0.5
    assert max(err_rect) <= MAX_TRANSLATION_ERROR, err_rect
