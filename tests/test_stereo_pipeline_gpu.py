"""MI355X: the semi-global matching op as a depth source.  pipeline.NetNodes(depth_source="stereo") builds no MonoDepth2 and hands over HipOps.stereo_sgm of the frame
and its right view, bit-equal to Context.stereo_sgm with graphs on and off; EndToEnd.push(right=...) parks that depth in the slot's ring buffer; the default
constructor still hands analyse_depth of its own depth_net the frame; and the tracker on the 12-frame Scene3D clip of tests/test_dis_pipeline_gpu.py with the op's
disparity image as the depth (KITTI ChooseData code, DepthMapFactor: 1, Camera.bf = fx * baseline = 250).  Each GPU step runs under a time limit of its own (limit());
ONE NetNodes of each kind is built in this file.

The tracker condition — translation error <= 0.05 m on every frame, the project's bar for a usable map source on this clip (test_dis_pipeline_gpu.py's
MAX_TRANSLATION_ERROR, under 2 % of the 3 m path) — is what "usable" means for this depth source; profiles/r25/stereo_tracker_gpu.txt keeps the series of a run."""
import os

import numpy as np
import pytest
import torch

from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

N_TRACK = 12
MAX_TRANSLATION_ERROR = 0.05
BASELINE = 0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(max_disp=64, p2=100)


def _bgr_stereo(vido, k=1):
    """A rectified pair of the convoy scene as BGR with channels that differ (so that the grey conversion matters); the channels are shifted along y only"""
    left, right, _, _ = vido.synth.convoy_scene(4).stereo_frame(k, 0.3)
    bgr = lambda g: np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=0), 255 - g], axis=-1))
    return bgr(left), bgr(right)


@pytest.fixture(scope="module")
def stereo_nodes(vido):
    from vido_slam_amd import pipeline
    with limit(600, "building NetNodes(depth_source='stereo')"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, depth_source="stereo", stereo_params=PARAMS)
        torch.cuda.synchronize()
    return nodes


def test_netnodes_with_the_op_as_depth_source(vido, stereo_nodes):
    nodes = stereo_nodes
    a, r = _bgr_stereo(vido)
    assert nodes.depth_net is None and nodes.depth_source == "stereo" and nodes.stereo_params == PARAMS
    assert not any(type(m).__name__ == "MonoDepth2" for m in vars(nodes).values())
    assert nodes.g_depth is not None, nodes.graph_error
    ref = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    want = ref.stereo_sgm(a, r, **PARAMS)
    want_rev = ref.stereo_sgm(r, a, **PARAMS)
    ref.close()
    ta, tr = torch.as_tensor(a, device="cuda"), torch.as_tensor(r, device="cuda")
    with pytest.raises(ValueError):
        nodes.infer(ta, ta)                                                         # no right view: refused before anything is enqueued
    with limit(120, "infer() with the depth graph, then eagerly"):
        got = []
        for k, (left, right) in enumerate(((ta, tr), (tr, ta), (ta, tr))):
            if k == 2:
                g_depth, nodes.g_depth = nodes.g_depth, None                        # the same nodes without the depth's graph
            flow, depth, mask, labels, evs = nodes.infer(left, left, right_bgr=right)
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            torch.cuda.synchronize()
            assert depth.dtype == torch.float32 and tuple(depth.shape) == (480, 640)
            got.append((depth.cpu().numpy().copy(), nodes.stereo_status.cpu().numpy().copy()))
        nodes.g_depth = g_depth
    for (d, s), w_ in zip(got, (want, want_rev, want)):
        assert np.array_equal(d, w_[0]) and np.array_equal(s, w_[2])
    assert want[3][0] > 0.5 * 640 * 480 and not np.array_equal(want[0], want_rev[0])


def test_end_to_end_parks_the_ops_depth(vido, stereo_nodes, tmp_path):
    from vido_slam_amd import pipeline
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    scene = vido.synth.convoy_scene(5)
    frames = [scene.frame(k) for k in range(3)]
    pairs = [scene.stereo_frame(k, 0.3)[:2] for k in range(3)]
    ref = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    want = [ref.stereo_sgm(vido.synth.gray_to_bgr(l_), vido.synth.gray_to_bgr(r_), **PARAMS)[0] for l_, r_ in pairs]
    ref.close()
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    e2e = pipeline.EndToEnd(stereo_nodes, slam, n_image=10 ** 6, feed="given")
    try:
        with pytest.raises(ValueError):
            e2e.push(vido.synth.gray_to_bgr(frames[0][0]), None)                    # stereo nodes: a frame without its right view is refused
        with limit(180, "3 frames of EndToEnd over the stereo nodes"):
            for k in range(3):
                g, d, f, m = frames[k]
                e2e.push(vido.synth.gray_to_bgr(g), (np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)),
                         right=vido.synth.gray_to_bgr(pairs[k][1]))
            e2e.finish()
            torch.cuda.synchronize()
            parked = [e2e.dev[k]["depth"].cpu().numpy() for k in range(3)]
    finally:
        e2e.close(); slam.close()
    assert e2e.err is None and len(e2e.poses) == 3
    for k in range(3):
        assert np.array_equal(parked[k], want[k]), k
    assert (want[1] > 0).mean() > 0.5


def test_default_constructor_runs_analyse_depth_of_its_own_depth_net(vido, monkeypatch):
    """depth_source defaults to "net": MonoDepth2 is built as before and the nodes' depth function is nets.analyse_depth of their own depth_net on the frame handed in —
    shown exactly, by identity: with the graph set aside and analyse_depth replaced by a recorder, infer() returns the recorder's tensor and the recorder saw depth_net,
    the frame and the nodes' feed and ops.  A right view is refused."""
    from vido_slam_amd import pipeline
    a, r = _bgr_stereo(vido)
    with limit(600, "building NetNodes()"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640)
        torch.cuda.synchronize()
    assert nodes.depth_source == "net" and nodes.stereo_params == {} and nodes.stereo_status is None
    assert type(nodes.depth_net).__name__ == "MonoDepth2" and nodes.g_depth is not None, nodes.graph_error
    ta, tr = torch.as_tensor(a, device="cuda"), torch.as_tensor(r, device="cuda")
    with pytest.raises(ValueError):
        nodes.infer(ta, ta, right_bgr=tr)
    seen = []; token = torch.full((480, 640), 7.0, device="cuda")
    monkeypatch.setattr(pipeline._nets, "analyse_depth", lambda net, x, **kw: (seen.append((net, x, kw)), token)[1])
    g_depth, nodes.g_depth = nodes.g_depth, None
    with limit(120, "infer() with the recorder"):
        depth = nodes.infer(ta, ta)[1]
        torch.cuda.synchronize()
    nodes.g_depth = g_depth
    assert depth is token and len(seen) == 1 and seen[0][0] is nodes.depth_net and seen[0][1] is ta
    assert seen[0][2] == dict(feed=nodes.depth_feed, ops=nodes.ops)


def _stereo_settings(tmp, scene, name):
    """Settings of this test's own: the KITTI ChooseData code (the depth image is a disparity: metres = bf / (raw / DepthMapFactor)), DepthMapFactor 1, bf = fx * baseline"""
    fx, fy, cx, cy = scene.K
    p = os.path.join(str(tmp), name)
    with open(p, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (scene.w, scene.h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: %.1f\nCamera.fps: 10.0\nCamera.RGB: 0\nChooseData: 2\nDepthMapFactor: 1\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n" % (fx * BASELINE))
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n")
    return p


def test_tracker_on_the_ops_depth(vido, tmp_path):
    """The 12-frame Scene3D clip of tests/test_dis_pipeline_gpu.py::test_tracker_on_the_ops_flow through System.TrackRGBD, the depth of frame k being the op's disp_out of
    stereo_frame(k, 0.5) at the defaults under settings of its own (KITTI code, DepthMapFactor: 1, Camera.bf: 250.0), with the rendered flow and mask; beside it the same
    clip with the rendered depth.  Condition: the camera's translation error is <= 0.05 m at every frame.

    Measured on an MI355X (profiles/r25/stereo_tracker_gpu.txt): translation error at the last frame 0.0071 m with the op's depth (the largest of the clip; met), 0.0038 m
    with the rendered depth; the op marks 0.926-0.941 of all pixels valid, with a median disparity error of 0.09-0.21 px on those."""
    from test_verify_flow_gpu import _settings, _track
    scene = vido.synth.Scene3D(n_frames=N_TRACK + 2, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    assert scene.K[0] * BASELINE == 250.0
    frames = [scene.frame(k) for k in range(N_TRACK)]
    ctx = vido.Context(width=640, height=480, max_batch=1)
    lines = []
    with limit(120, "the op's disparity of 12 stereo pairs"):
        sgm, share, med = [], [], []
        for k in range(N_TRACK):
            left, right, depth, mask = scene.stereo_frame(k, BASELINE)
            assert np.array_equal(left, frames[k][0])
            disp, q4, status, stats = ctx.stereo_sgm(left, right)
            true = scene.K[0] * BASELINE / depth.astype(np.float64)
            ok = status == 0
            share.append(float(ok.mean())); med.append(float(np.median(np.abs(disp[ok] - true[ok]))))
            sgm.append((frames[k][0], disp, frames[k][2], frames[k][3]))
        ctx.close()
    lines.append("vido_stereo_sgm at the defaults against Scene3D's disparity (baseline %.1f m, bf 250), all pixels, per frame: share with status 0 " % BASELINE
                 + " ".join("%.3f" % s for s in share) + "; median |error| px of those " + " ".join("%.3f" % m for m in med))
    with limit(120, "12 frames, the rendered depth"):
        _, err_true, _ = _track(vido, _settings(tmp_path, scene, "true.yaml"), scene, frames, N_TRACK)
    with limit(120, "12 frames, the op's disparity as the depth"):
        _, err_sgm, _ = _track(vido, _stereo_settings(tmp_path, scene, "stereo.yaml"), scene, sgm, N_TRACK)
    lines.append("translation error m, rendered depth:       " + " ".join("%.4f" % e for e in err_true))
    lines.append("translation error m, vido_stereo_sgm:      " + " ".join("%.4f" % e for e in err_sgm))
    lines.append("condition: translation error <= %.2f m at every frame with vido_stereo_sgm: max %.4f m -> %s" % (
        MAX_TRANSLATION_ERROR, max(err_sgm), "met" if max(err_sgm) <= MAX_TRANSLATION_ERROR else "MISSED"))
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r25"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r25", "stereo_tracker_gpu.txt"), "w") as fh:
            fh.write("tests/test_stereo_pipeline_gpu.py::test_tracker_on_the_ops_depth — Scene3D(seed 3, one object), 12 frames, 640 x 480, MI355X\n" + "\n".join(lines) + "\n")
    except OSError:
        pass                                                                      # (a read-only tree: the figures are printed above)
    assert min(share) > 0.5
    assert max(err_sgm) <= MAX_TRANSLATION_ERROR, err_sgm
