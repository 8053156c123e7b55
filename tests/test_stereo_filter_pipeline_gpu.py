"""MI355X: the speckle filter inside the network nodes, and the stereo depth deciding label collisions.  One module-scoped
NetNodes(flow_source="dis", depth_source="stereo", detect_every=2, stereo_filter=True, propagate_bf=250): infer()'s depth and stereo_status equal the numpy statements of
vido_stereo_sgm and vido_stereo_filter chained; on a propagated frame a 1-pixel checker of labels 1 / 2 written into carried_mask comes back as the statement of
vido_mask_propagate with the PREVIOUS frame's collision depth, bit for bit, and that differs from the statement without a depth (else the test fails as vacuous); InstanceIds hands a depth on the same way; the
constructor's refusals; nodes built without the two arguments hold no filter state and pass no depth; and the tracker on the 12-frame Scene3D clip of
tests/test_stereo_pipeline_gpu.py with the filtered disparity (translation error <= 0.05 m on every frame, the project's bar on this clip).  Each GPU step runs under
limit().  profiles/r26/stereo_filter_tracker_gpu.txt keeps the tracker's series of a run, with and without the filter: whether the filter helps the pose is a finding."""
import os

import numpy as np
import pytest
import torch

from refimpl import mask_propagate_np as MP
from refimpl import stereo_filter_np as F
from refimpl import stereo_sgm_np as G
from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

N_TRACK = 12
MAX_TRANSLATION_ERROR = 0.05
BASELINE = 0.5
BF = 250.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(max_disp=64)                                                        # (half the volume of the default: the numpy statement of one 640 x 480 pair in seconds)


def _scene(vido, n=4):
    return vido.synth.Scene3D(n_frames=n, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))


@pytest.fixture(scope="module")
def nodes(vido):
    from vido_slam_amd import pipeline
    with limit(600, "building NetNodes(stereo_filter=True, propagate_bf=250)"):
        n = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, flow_source="dis", depth_source="stereo", stereo_params=PARAMS, detect_every=2,
                              stereo_filter=True, propagate_bf=BF)
        torch.cuda.synchronize()
    return n


@pytest.fixture(scope="module")
def statements(vido):
    """frame 0 of the clip: (left, right) BGR and the two statements chained on it — computed once"""
    scene = _scene(vido)
    left, right, _, _ = scene.stereo_frame(0, BASELINE)
    _, q4, status, _ = G.stereo_sgm(left, right, **{**G.DEFAULTS, **PARAMS})
    disp, st, depth, stats = F.stereo_filter(q4, status, bf=BF, **F.DEFAULTS)
    return scene, vido.synth.gray_to_bgr(left), vido.synth.gray_to_bgr(right), (disp, st, depth, stats), status


def test_depth_status_and_collision_depth_through_infer(vido, nodes, statements):
    scene, left, right, (disp, st, plane, stats), sgm_status = statements
    assert nodes.stereo_filter == {} and nodes.propagate_bf == BF and nodes.g_depth is not None, nodes.graph_error
    assert stats[2] > 0 and (st == 4).sum() == stats[2] and (sgm_status != 4).all()      # the filter removes something on this pair
    checker = ((np.add.outer(np.arange(480), np.arange(640)) & 1) + 1).astype(np.int32)
    nxt = scene.stereo_frame(1, BASELINE)
    tl, tr = torch.as_tensor(left, device="cuda"), torch.as_tensor(right, device="cuda")
    tl1, tr1 = torch.as_tensor(vido.synth.gray_to_bgr(nxt[0]), device="cuda"), torch.as_tensor(vido.synth.gray_to_bgr(nxt[1]), device="cuda")
    seen = []
    real = nodes.ops.mask_propagate
    nodes.ops.mask_propagate = lambda mask, flow, depth=None, **kw: (seen.append(depth), real(mask, flow, depth=depth, **kw))[1]
    try:
        with limit(120, "a detector frame and a propagated frame through infer()"):
            nodes._set_detect_every(2)                                              # a new sequence: the first frame passes no depth
            flow, depth, mask, labels, evs = nodes.infer(tl, tl, right_bgr=tr)
            torch.cuda.synchronize()
            assert not nodes.last_propagated and seen == []
            got = depth.cpu().numpy().copy(), nodes.stereo_status.cpu().numpy().copy(), nodes._coll[nodes._coll_i].cpu().numpy().copy()
            nodes.carried_mask.copy_(torch.as_tensor(checker, device="cuda"))
            flow, depth, mask, labels, evs = nodes.infer(tl, tl1, right_bgr=tr1)
            torch.cuda.synchronize()
            assert nodes.last_propagated and len(seen) == 1 and seen[0] is not None
            prev_plane = seen[0].cpu().numpy().copy(); flow_np = flow.cpu().numpy().copy(); mask_np = mask.cpu().numpy().copy()
            st1 = nodes.stereo_status.cpu().numpy().copy()
    finally:
        nodes.ops.mask_propagate = real
    # the two statements chained, bit for bit; the plane the next frame's propagation received is this frame's
    assert got[0].tobytes() == disp.tobytes() and np.array_equal(got[1], st) and got[2].tobytes() == plane.tobytes()
    assert prev_plane.tobytes() == plane.tobytes()
    assert (st1 == 4).any() and (got[1] == 4).any()
    want, _ = MP.propagate(checker, flow_np, depth_prev=plane)
    plain, _ = MP.propagate(checker, flow_np)
    print("propagated frame: %d labelled pixels, %d differ between the statement with the stereo depth and without" % ((want > 0).sum(), (want != plain).sum()))
    assert (want != plain).any(), "vacuous: on this pair the depth decides no collision"
    assert np.array_equal(mask_np, want)


def test_instance_ids_hand_the_depth_to_mask_propagate(vido, statements):
    """InstanceIds (what NetNodes(stable_ids=True) drives): propagated(flow, depth=) is the statement of vido_mask_propagate with that depth, and detected(..., depth=)
    hands the same tensor to its mask_propagate call; without the argument no depth is passed."""
    from vido_slam_amd import nets, pipeline
    scene, _, _, (_, _, plane, _), _ = statements
    checker = ((np.add.outer(np.arange(480), np.arange(640)) & 1) + 1).astype(np.int32)
    flow = np.ascontiguousarray(scene.frame(0)[2], np.float32)
    want, _ = MP.propagate(checker, flow, depth_prev=plane)
    plain, _ = MP.propagate(checker, flow)
    assert (want != plain).any(), "vacuous: the depth decides no collision"
    ctx = vido.Context(width=640, height=480, max_batch=1)
    ops = nets.HipOps(ctx)
    seen = []
    real = ops.mask_propagate
    ops.mask_propagate = lambda mask, flow, depth=None, **kw: (seen.append(depth), real(mask, flow, depth=depth, **kw))[1]
    try:
        with limit(120, "InstanceIds with a depth"):
            ids = pipeline.InstanceIds(ops, 480, 640)
            tf, tp, tc = torch.as_tensor(flow, device="cuda"), torch.as_tensor(plane, device="cuda"), torch.as_tensor(checker, device="cuda")
            del seen[:]
            ids.mask.copy_(tc)
            got = ids.propagated(tf, depth=tp).cpu().numpy()
            ids.mask.copy_(tc)
            got_plain = ids.propagated(tf).cpu().numpy()
            inst = torch.zeros((480, 640), dtype=torch.int32, device="cuda"); classes = torch.zeros((127,), dtype=torch.int64, device="cuda")
            ids.detected(inst, classes, tf, depth=tp)
            ids.detected(inst, classes, tf)
            ids.detected(inst, classes, None, depth=tp)                             # the first frame of a sequence: nothing is warped
            torch.cuda.synchronize()
    finally:
        ctx.close()
    assert np.array_equal(got, want) and np.array_equal(got_plain, plain)
    assert len(seen) == 4 and seen[0] is tp and seen[1] is None and seen[2] is tp and seen[3] is None


def test_constructor_refusals(vido):
    from vido_slam_amd import pipeline
    ctx = vido.Context(width=640, height=480, max_batch=1)
    base = dict(flow_source="dis", depth_source="stereo", detect_every=2)
    bad = [dict(base, depth_source="net", stereo_filter=True), dict(base, stereo_filter=False), dict(base, stereo_filter=1), dict(base, stereo_filter="on"),
           dict(base, stereo_filter=dict(min_area=3)), dict(base, stereo_filter=dict(min_region=2.5)), dict(base, stereo_filter=dict(min_region=True)),
           dict(base, stereo_filter=dict(min_region=0)), dict(base, stereo_filter=dict(min_region=(1 << 24) + 1)), dict(base, stereo_filter=dict(max_diff_q4=-1)),
           dict(base, stereo_filter=dict(max_diff_q4=65536)),
           dict(base, propagate_bf=0.0), dict(base, propagate_bf=-3.0), dict(base, propagate_bf=float("inf")), dict(base, propagate_bf=float("nan")), dict(base, propagate_bf="250"),
           dict(base, propagate_bf=True), dict(base, depth_source="net", propagate_bf=250.0), dict(base, detect_every=1, propagate_bf=250.0)]
    try:
        for kw in bad:
            with pytest.raises(ValueError):
                pipeline.NetNodes(ctx, 480, 640, **kw)
        C_ = pipeline.NetNodes._check_stereo_filter
        assert C_(None, None, "net", 1, False) == (None, None)
        assert C_(True, None, "stereo", 1, False) == ({}, None)
        assert C_(dict(max_diff_q4=8, min_region=25), 250, "stereo", 2, False) == (dict(max_diff_q4=8, min_region=25), 250.0)
        assert C_(None, 75.5, "stereo", 1, True) == (None, 75.5)
    finally:
        ctx.close()


def test_without_the_arguments_no_filter_state_and_no_depth(vido, statements):
    """The two arguments default to None: the nodes hold no filter state, the depth function is the SGM call alone, and mask_propagate receives no depth."""
    from vido_slam_amd import pipeline
    scene, left, right, _, sgm_status = statements
    with limit(600, "building NetNodes(depth_source='stereo', detect_every=2)"):
        n = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, flow_source="dis", depth_source="stereo", stereo_params=PARAMS, detect_every=2,
                              graphs=False, calibrate_scores=False)
        torch.cuda.synchronize()
    assert n.stereo_filter is None and n.propagate_bf is None and n._coll is None and n._coll_static is None and not hasattr(n, "_stereo_q4")
    seen = []
    real = n.ops.mask_propagate
    n.ops.mask_propagate = lambda mask, flow, depth=None, **kw: (seen.append(depth), real(mask, flow, depth=depth, **kw))[1]
    filt = []
    n.ops.stereo_filter = lambda *a, **kw: filt.append(a)
    tl, tr = torch.as_tensor(left, device="cuda"), torch.as_tensor(right, device="cuda")
    with limit(120, "two frames through infer()"):
        for _ in range(2):
            n.infer(tl, tl, right_bgr=tr)
        torch.cuda.synchronize()
        status = n.stereo_status.cpu().numpy()
    assert n.last_propagated and seen == [None] and filt == []
    assert np.array_equal(status, sgm_status)                                      # SGM's own status: no 4 anywhere


def _stereo_settings(tmp, scene, name):
    from test_stereo_pipeline_gpu import _stereo_settings as s
    return s(tmp, scene, name)


def test_tracker_on_the_filtered_depth(vido, tmp_path):
    """The 12-frame Scene3D clip of tests/test_stereo_pipeline_gpu.py::test_tracker_on_the_ops_depth with the filter at its defaults behind vido_stereo_sgm, and beside it
    without.  Conditions: every pose finite, translation error <= 0.05 m at every frame with the filter on."""
    from test_verify_flow_gpu import _track
    scene = _scene(vido, N_TRACK + 2)
    frames = [scene.frame(k) for k in range(N_TRACK)]
    ctx = vido.Context(width=640, height=480, max_batch=1)
    lines = []
    with limit(120, "the op's disparity of 12 stereo pairs, filtered and not"):
        plain, filtered, removed = [], [], []
        for k in range(N_TRACK):
            left, right, depth, mask = scene.stereo_frame(k, BASELINE)
            disp, q4, status, stats = ctx.stereo_sgm(left, right)
            fdisp, fstatus, _, fstats = ctx.stereo_filter(q4, status)
            assert np.array_equal(fdisp[fstatus == 0], disp[fstatus == 0]) and (fdisp[fstatus != 0] == -1).all() and fstats[0] == stats[0]
            removed.append(int(fstats[2]))
            plain.append((frames[k][0], disp, frames[k][2], frames[k][3])); filtered.append((frames[k][0], fdisp, frames[k][2], frames[k][3]))
        ctx.close()
    lines.append("vido_stereo_filter at the defaults %s behind vido_stereo_sgm at its defaults, pixels removed per frame: %s" % (F.DEFAULTS, " ".join(map(str, removed))))
    with limit(120, "12 frames, the op's disparity"):
        _, err_plain, _ = _track(vido, _stereo_settings(tmp_path, scene, "plain.yaml"), scene, plain, N_TRACK)
    with limit(120, "12 frames, the filtered disparity"):
        poses, err_filt, _ = _track(vido, _stereo_settings(tmp_path, scene, "filtered.yaml"), scene, filtered, N_TRACK)
    lines.append("translation error m, vido_stereo_sgm:                       " + " ".join("%.4f" % e for e in err_plain))
    lines.append("translation error m, vido_stereo_sgm + vido_stereo_filter:  " + " ".join("%.4f" % e for e in err_filt))
    lines.append("condition: translation error <= %.2f m at every frame with the filter: max %.4f m -> %s (without: max %.4f m)" % (
        MAX_TRANSLATION_ERROR, max(err_filt), "met" if max(err_filt) <= MAX_TRANSLATION_ERROR else "MISSED", max(err_plain)))
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r26"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r26", "stereo_filter_tracker_gpu.txt"), "w") as fh:
            fh.write("tests/test_stereo_filter_pipeline_gpu.py::test_tracker_on_the_filtered_depth — Scene3D(seed 3, one object), 12 frames, 640 x 480, MI355X\n" + "\n".join(lines) + "\n")
    except OSError:
        pass                                                                      # (a read-only tree: the figures are printed above)
    assert sum(removed) > 0
    assert all(np.isfinite(T).all() for T in poses)
    assert max(err_filt) <= MAX_TRANSLATION_ERROR, err_filt
