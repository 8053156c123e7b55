"""MI355X: the forward-backward check in the pipeline.  pipeline.NetNodes(flow_source="dis", dis_consistency=True) hands over HipOps.dis_flow_pair's marked flow — bit-equal to
the two statements (tests/refimpl/dis_flow_np.py in both directions, tests/refimpl/flow_consistency_np.py on the two fields), captured and eager — and exposes the status
image; with dis_consistency=None the flow function is HipOps.dis_flow as before; and the tracker on the 12-frame Scene3D clip of tests/test_dis_pipeline_gpu.py with the
marked flow.  Each GPU step runs under a time limit of its own (limit()).

The tracker conditions are those of the unmarked flow — finite poses, translation error <= 0.05 m at every frame — plus a non-empty static set on every frame the true-flow
run has one: a flow with NaN holes must still be usable.  Whether the marking helps or hurts the pose is recorded, not barred: profiles/r21/dis_consistency_tracker_gpu.txt
keeps the series of a run."""
import os

import numpy as np
import pytest
import torch

from refimpl import dis_flow_np as D
from refimpl import flow_consistency_np as F
from test_detect_every_gpu import limit
from test_dis_pipeline_gpu import _bgr_pair, N_TRACK, MAX_TRANSLATION_ERROR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dis_consistency_argument_checks():
    """Refused before any network is built (no GPU work: the checks come first)."""
    from vido_slam_amd import pipeline
    for bad in (False, 1, "on", [10, 32768], dict(alpha=10), dict(alpha_q10=10.0), dict(alpha_q10=True), dict(alpha_q10=1025), dict(beta_q16=-1), dict(beta_q16=(1 << 30) + 1),
                dict(alpha_q10=10, coarsest=3)):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, flow_source="dis", dis_consistency=bad)
    for cons in (True, {}, dict(alpha_q10=10)):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, flow_source="net", dis_consistency=cons)
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, dis_consistency=cons)
    assert pipeline.NetNodes._check_dis_consistency(None, "dis") is None and pipeline.NetNodes._check_dis_consistency(None, "net") is None
    assert pipeline.NetNodes._check_dis_consistency(True, "dis") == {} and pipeline.NetNodes._check_dis_consistency(dict(beta_q16=8192), "dis") == dict(beta_q16=8192)


def test_netnodes_hand_over_the_marked_flow(vido):
    from vido_slam_amd import pipeline
    a, b = _bgr_pair(vido)
    params = dict(coarsest=3, iters=4); cons = dict(beta_q16=16384)
    with limit(600, "building NetNodes(flow_source='dis', dis_consistency=...)"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, flow_source="dis", dis_params=params, dis_consistency=cons, detect_every=2)
        torch.cuda.synchronize()
    assert nodes.flow_net is None and nodes.dis_consistency == cons and nodes.g_flow is not None, nodes.graph_error
    assert nodes.flow_status is not None and nodes.flow_status.dtype == torch.uint8 and tuple(nodes.flow_status.shape) == (480, 640)
    want = {}
    q8 = {"ab": D.dis_flow(a, b, **params)[1], "ba": D.dis_flow(b, a, **params)[1]}           # (each field is the other order's backward field)
    for key, back in (("ab", "ba"), ("ba", "ab")):
        want[key] = F.flow_consistency(q8[key], q8[back], beta_q16=16384)
        print("%s: check stats %s" % (key, want[key][2].tolist()))
        assert (want[key][2][:3] > 0).all()
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    with limit(120, "infer() with the flow graph, then eagerly, detect_every = 2"):
        for k, (p, c, key) in enumerate(((ta, tb, "ab"), (tb, ta, "ba"), (ta, tb, "ab"), (tb, ta, "ba"))):
            if k == 2:
                g_flow, nodes.g_flow = nodes.g_flow, None                       # the same nodes without the flow's graph
            flow, depth, mask, labels, evs = nodes.infer(p, c)
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            torch.cuda.synchronize()
            status, marked, stats = want[key]
            assert flow.dtype == torch.float32 and tuple(flow.shape) == (480, 640, 2)
            assert np.array_equal(flow.cpu().numpy().view(np.uint32), marked.view(np.uint32)), (k, key)
            assert np.array_equal(nodes.flow_status.cpu().numpy(), status), (k, key)
            assert bool(torch.isnan(flow).any(-1).eq(nodes.flow_status != 0).all())
            assert mask.dtype == torch.int32 and tuple(mask.shape) == (480, 640)   # (odd calls carry the mask through the marked flow: NaN sources do not vote)
        nodes.g_flow = g_flow
    assert nodes.detector_runs == 2 and nodes.propagated_frames == 2


def test_off_is_the_single_direction_op(vido, monkeypatch):
    """dis_consistency=None: the nodes' flow function is HipOps.dis_flow with the nodes' parameters, shown by identity with a recorder in its place, and its result equals
    Context.dis_flow; dis_flow_pair is never called."""
    from vido_slam_amd import pipeline
    a, b = _bgr_pair(vido)
    params = dict(coarsest=3, iters=4)
    with limit(600, "building NetNodes(flow_source='dis')"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, flow_source="dis", dis_params=params)
        torch.cuda.synchronize()
    assert nodes.dis_consistency is None and nodes.flow_status is None and nodes.g_flow is not None, nodes.graph_error
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    ref = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    want = ref.dis_flow(a, b, **params)[0]
    ref.close()
    with limit(120, "the flow function, eager and captured"):
        got = nodes._flow_fn(ta, tb); torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
        flow = nodes.infer(ta, tb)[0]; torch.cuda.synchronize()
        assert np.array_equal(flow.cpu().numpy(), want)
    seen = []; token = torch.full((480, 640, 2), 7.0, device="cuda")
    monkeypatch.setattr(nodes.ops_flow, "dis_flow", lambda x, y, **kw: (seen.append((x, y, kw)), token)[1])
    monkeypatch.setattr(nodes.ops_flow, "dis_flow_pair", lambda *x, **kw: pytest.fail("dis_flow_pair called with dis_consistency=None"))
    assert nodes._flow_fn(ta, tb) is token and len(seen) == 1 and seen[0][0] is ta and seen[0][1] is tb and seen[0][2] == params


def test_tracker_on_the_marked_flow(vido, tmp_path):
    """The 12-frame Scene3D clip of tests/test_dis_pipeline_gpu.py::test_tracker_on_the_ops_flow through System.TrackRGBD, the flow of frame k being Context.dis_flow_pair's
    marked flow of the grey images k and k + 1 at the defaults; beside it the unmarked flow (the pair call's forward field) and the true flow.  Conditions: every pose
    finite, translation error <= 0.05 m at every frame, n_static > 0 on every frame on which the true-flow run has a static set.  Recorded without a bar: the error per
    frame of the three runs and the share of pixels marked.

    Measured on an MI355X (profiles/r21/dis_consistency_tracker_gpu.txt): 0.19 of the pixels marked (0.11-0.17 inconsistent, 0.05-0.06 leaving the image); translation error
    at the last frame, the largest of each run: 0.0161 m with the marked flow (met), 0.0115 m unmarked, 0.0038 m with the true flow — the marking leaves the pose error
    HIGHER, on every frame from the second on; n_static 1586 / 1973 / 2196 on frames 0-2 against 1771 / 2211 / 2529 unmarked, the cap of 3000 from frame 8 against 5."""
    from test_verify_flow_gpu import _settings, _track
    scene = vido.synth.Scene3D(n_frames=N_TRACK + 2, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = [scene.frame(k) for k in range(N_TRACK + 1)]
    ctx = vido.Context(width=640, height=480, max_batch=1)
    lines = []
    with limit(120, "the pair op on 12 frame pairs"):
        marked, plain, share = [], [], []
        for k in range(N_TRACK):
            flow, fwd, bwd, status, stats = ctx.dis_flow_pair(frames[k][0], frames[k + 1][0])
            assert np.array_equal(np.isnan(flow).any(-1), status != 0)
            share.append([float(stats[8 + j]) / status.size for j in range(4)])
            marked.append((frames[k][0], frames[k][1], flow, frames[k][3]))
            plain.append((frames[k][0], frames[k][1], fwd.astype(np.float32) / np.float32(256), frames[k][3]))
        ctx.close()
    lines.append("share of pixels per frame pair, status 1 (inconsistent): " + " ".join("%.3f" % s[1] for s in share))
    lines.append("share of pixels per frame pair, status 2 (leaves the image): " + " ".join("%.3f" % s[2] for s in share))
    lines.append("share of pixels marked NaN, mean over the clip: %.3f" % float(np.mean([1.0 - s[0] for s in share])))
    true = [frames[k] for k in range(N_TRACK)]
    with limit(120, "12 frames, the true flow"):
        _, err_true, st_true = _track(vido, _settings(tmp_path, scene, "true.yaml"), scene, true, N_TRACK)
    with limit(120, "12 frames, the unmarked flow"):
        _, err_plain, st_plain = _track(vido, _settings(tmp_path, scene, "plain.yaml"), scene, plain, N_TRACK)
    with limit(120, "12 frames, the marked flow"):
        poses, err_mark, st_mark = _track(vido, _settings(tmp_path, scene, "marked.yaml"), scene, marked, N_TRACK)
    lines.append("translation error m, true flow:                 " + " ".join("%.4f" % e for e in err_true))
    lines.append("translation error m, vido_dis_flow (unmarked):  " + " ".join("%.4f" % e for e in err_plain))
    lines.append("translation error m, vido_dis_flow_pair marked: " + " ".join("%.4f" % e for e in err_mark))
    for name, st in (("true flow", st_true), ("unmarked", st_plain), ("marked", st_mark)):
        lines.append("n_static / n_static_inliers / n_object_points, %-9s " % (name + ":") + " ".join("%d/%d/%d" % (s["n_static"], s["n_static_inliers"], s["n_object_points"]) for s in st))
    verdict = "lower" if max(err_mark) < max(err_plain) else "higher" if max(err_mark) > max(err_plain) else "equal"
    lines.append("largest error of the clip: marked %.4f m, unmarked %.4f m, true flow %.4f m: the marking leaves the pose error %s" % (max(err_mark), max(err_plain), max(err_true), verdict))
    lines.append("condition: translation error <= %.2f m at every frame with the marked flow: max %.4f m -> %s" % (MAX_TRANSLATION_ERROR, max(err_mark), "met" if max(err_mark) <= MAX_TRANSLATION_ERROR else "MISSED"))
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r21"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r21", "dis_consistency_tracker_gpu.txt"), "w") as fh:
            fh.write("tests/test_dis_consistency_pipeline_gpu.py::test_tracker_on_the_marked_flow — Scene3D(seed 3, one object), 12 frames, 640 x 480, MI355X\n" + "\n".join(lines) + "\n")
    except OSError:
        pass                                                                      # (a read-only tree: the figures are printed above)
    assert all(np.isfinite(T).all() for T in poses)
    assert max(err_mark) <= MAX_TRANSLATION_ERROR, err_mark
    assert all(m["n_static"] > 0 for m, t in zip(st_mark, st_true) if t["n_static"] > 0), [m["n_static"] for m in st_mark]
