"""MI355X: the dense inverse-search flow op as a flow source.  pipeline.NetNodes(flow_source="dis") builds no LiteFlowNet and hands over HipOps.dis_flow of the two BGR
frames, bit-equal to Context.dis_flow with graphs on and off; the default constructor still hands over its own LiteFlowNet's flow; and the tracker on the 12-frame Scene3D
clip of tests/test_verify_flow_gpu.py with the op's flow in place of the rendered one.  Each GPU step runs under a time limit of its own (limit()).

The tracker condition — translation error <= 0.05 m on every frame, under 2 % of the 3 m path, where the true-flow run sits at 0.003-0.006 m — is what "usable" means for
this flow source; profiles/r20/dis_tracker_gpu.txt keeps the series of a run."""
import os

import numpy as np
import pytest
import torch

from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

N_TRACK = 12
MAX_TRANSLATION_ERROR = 0.05
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bgr_pair(vido, k=1):
    """Two frames of the convoy scene as BGR with channels that differ (so that the grey conversion matters)"""
    scene = vido.synth.convoy_scene(4)
    out = []
    for j in (k, k + 1):
        g = scene.frame(j)[0]
        out.append(np.ascontiguousarray(np.stack([g, np.roll(g, 1, axis=1), 255 - g], axis=-1)))
    return out


def test_netnodes_with_the_op_as_flow_source(vido):
    from vido_slam_amd import pipeline
    a, b = _bgr_pair(vido)
    params = dict(coarsest=3, iters=4)
    with limit(600, "building NetNodes(flow_source='dis', detect_every=2)"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, flow_source="dis", dis_params=params, detect_every=2)
        torch.cuda.synchronize()
    assert nodes.flow_net is None and nodes.flow_source == "dis"
    assert not any(type(m).__name__ == "LiteFlowNet" for m in vars(nodes).values())
    assert nodes.g_flow is not None, nodes.graph_error
    ref = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    want = ref.dis_flow(a, b, **params)[0]
    want_rev = ref.dis_flow(b, a, **params)[0]
    ref.close()
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    with limit(120, "infer() with the flow graph, then eagerly, detect_every = 2"):
        got = []
        for k, (p, c) in enumerate(((ta, tb), (tb, ta), (ta, tb))):
            if k == 2:
                g_flow, nodes.g_flow = nodes.g_flow, None                       # the same nodes without the flow's graph
            flow, depth, mask, labels, evs = nodes.infer(p, c)
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            torch.cuda.synchronize()
            assert flow.dtype == torch.float32 and tuple(flow.shape) == (480, 640, 2)
            got.append(flow.cpu().numpy().copy())
        nodes.g_flow = g_flow
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want_rev) and np.array_equal(got[2], want)
    assert np.abs(want).max() > 0.5
    assert nodes.detector_runs == 2 and nodes.propagated_frames == 1               # calls 0 and 2 detect, call 1 carries the mask through the op's flow
    out = nodes.recompute(ta, tb, flow=True, detector=False)
    assert out["flow"] is None and nodes.range_recomputes["flow"] == 0             # nothing to recompute: the op has no range to leave


def test_flow_source_argument_checks():
    """Refused before any network is built (no GPU needed: the checks come first)."""
    from vido_slam_amd import pipeline
    for bad in ("lfn", "DIS", None, 1, ""):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, flow_source=bad)
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, flow_source="net", dis_params=dict(iters=4))
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, flow_source="dis", dis_params=dict(levels=4))
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, flow_source="dis", dis_params=[4])


def test_default_constructor_runs_analyse_flow_of_its_own_flow_net(vido, monkeypatch):
    """flow_source defaults to "net": LiteFlowNet is built as before and the nodes' flow function is nets.analyse_flow of their own flow_net on the two frames handed in —
    shown exactly, by identity: with the graph set aside and analyse_flow replaced by a recorder, infer() returns the recorder's tensor and the recorder saw flow_net and
    the two frames."""
    from vido_slam_amd import pipeline, nets
    a, b = _bgr_pair(vido)
    with limit(600, "building NetNodes()"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640)
        torch.cuda.synchronize()
    assert nodes.flow_source == "net" and nodes.dis_params == {} and type(nodes.flow_net).__name__ == "LiteFlowNet" and nodes.g_flow is not None, nodes.graph_error
    ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
    seen = []; token = torch.full((480, 640, 2), 7.0, device="cuda")
    monkeypatch.setattr(pipeline._nets, "analyse_flow", lambda net, x, y: (seen.append((net, x, y)), token)[1])
    g_flow, nodes.g_flow = nodes.g_flow, None
    with limit(120, "infer() with the recorder"):
        flow = nodes.infer(ta, tb)[0]
        torch.cuda.synchronize()
    nodes.g_flow = g_flow
    assert flow is token and len(seen) == 1 and seen[0][0] is nodes.flow_net and seen[0][1] is ta and seen[0][2] is tb


def test_default_constructor_still_hands_over_liteflownet(vido):
    """flow_source defaults to "net": the flow infer() returns is bit-equal to analyse_flow of the nodes' own flow_net, from the captured graph and, with the graph set
    aside, eagerly.

    The nodes are built and compared with torch.backends.cudnn.deterministic on (restored afterwards): a comparison to the bit needs convolutions that repeat to the bit,
    and in the library's default mode LiteFlowNet's do not.  Measured on an MI355X on the same pair, |flow| max 1.33 px: two calls of analyse_flow differ by up to 4.2e-6 px
    and a capture from an eager call by 3.5e-6, the first difference arising in a library convolution of the 15 x 20 level (netMatching.4.netFeat, 2.4e-7); with the
    switch on, eager against eager, capture against eager and capture against capture are all 0.  The switch changes which solver the library picks, nothing of ours."""
    from vido_slam_amd import pipeline, nets
    a, b = _bgr_pair(vido)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with limit(600, "building NetNodes()"):
            nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640)
            torch.cuda.synchronize()
        assert nodes.flow_source == "net" and type(nodes.flow_net).__name__ == "LiteFlowNet" and nodes.g_flow is not None, nodes.graph_error
        ta, tb = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")

        def infer():
            flow, depth, mask, labels, evs = nodes.infer(ta, tb)
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            torch.cuda.synchronize()
            return flow.clone()

        with limit(180, "infer() against analyse_flow, captured and eager"):
            got_graph = infer()
            g_flow, nodes.g_flow = nodes.g_flow, None
            got_eager = infer()
            nodes.g_flow = g_flow
            with torch.no_grad():
                want = nets.analyse_flow(nodes.flow_net, ta, tb).clone()
                again = nets.analyse_flow(nodes.flow_net, ta, tb)
            torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic = was
    print("largest |difference|: captured infer() against analyse_flow %.3g, eager infer() %.3g, analyse_flow against itself %.3g (|flow| max %.3g)" % (
        float((got_graph - want).abs().max()), float((got_eager - want).abs().max()), float((again - want).abs().max()), float(want.abs().max())))
    assert torch.equal(again, want)                                             # the premise: the reference repeats to the bit
    assert float(want.abs().max()) > 0.1
    assert torch.equal(got_graph, want)
    assert torch.equal(got_eager, want)


def test_tracker_on_the_ops_flow(vido, tmp_path):
    """The 12-frame Scene3D clip of tests/test_verify_flow_gpu.py through System.TrackRGBD the way its _track does, the flow of frame k being the op's flow of the grey images
    k and k + 1 at the defaults; beside it the same clip with the true flow.  Condition: the camera's translation error is <= 0.05 m at every frame.  Recorded without a
    bar: the run with Verify.Descriptor: 1 and Verify.ObjectPatch: 1, and the shares they reject.

    Measured on an MI355X (profiles/r20/dis_tracker_gpu.txt): translation error at the last frame 0.0115 m with the op's flow (the largest of the clip; met), 0.0038 m with
    the true flow, 0.0115 m with both guards on (0.020 m at frame 3); Verify.Descriptor rejects 0.075 of the static points, Verify.ObjectPatch 0.012 of the object points."""
    from test_verify_flow_gpu import _settings, _track, MAX_HAMMING
    scene = vido.synth.Scene3D(n_frames=N_TRACK + 2, seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    frames = [scene.frame(k) for k in range(N_TRACK + 1)]
    ctx = vido.Context(width=640, height=480, max_batch=1)
    lines = []
    with limit(120, "the op's flow of 12 frame pairs"):
        dis, epe = [], []
        for k in range(N_TRACK):
            f, q8, st = ctx.dis_flow(frames[k][0], frames[k + 1][0])
            e = np.hypot(f[..., 0] - frames[k][2][..., 0], f[..., 1] - frames[k][2][..., 1])
            epe.append((float(np.median(e)), float((e < 0.4).mean())))
            dis.append((frames[k][0], frames[k][1], f, frames[k][3]))
        ctx.close()
    lines.append("vido_dis_flow at the defaults against Scene3D's flow, all pixels, per frame pair: median EPE px " + " ".join("%.3f" % m for m, _ in epe) + "; share < 0.4 px " + " ".join("%.3f" % s for _, s in epe))
    true = [frames[k] for k in range(N_TRACK)]
    rej = {"desc": [0, 0], "patch": [0, 0, 0]}

    def count(k, slam, g):
        c, r = slam.verify_stats(); rej["desc"][0] += c; rej["desc"][1] += r
        c, r, nt = slam.object_verify_stats(); rej["patch"][0] += c; rej["patch"][1] += r; rej["patch"][2] += nt

    with limit(120, "12 frames, the true flow"):
        _, err_true, st_true = _track(vido, _settings(tmp_path, scene, "true.yaml"), scene, true, N_TRACK)
    with limit(120, "12 frames, the op's flow"):
        _, err_dis, st_dis = _track(vido, _settings(tmp_path, scene, "dis.yaml"), scene, dis, N_TRACK)
    with limit(120, "12 frames, the op's flow, Verify.Descriptor + Verify.ObjectPatch"):
        _, err_ver, st_ver = _track(vido, _settings(tmp_path, scene, "ver.yaml", "Verify.Descriptor: 1\nVerify.MaxHamming: %d\nVerify.ObjectPatch: 1\n" % MAX_HAMMING), scene, dis, N_TRACK, per_frame=count)
    lines.append("translation error m, true flow:                  " + " ".join("%.4f" % e for e in err_true))
    lines.append("translation error m, vido_dis_flow:              " + " ".join("%.4f" % e for e in err_dis))
    lines.append("translation error m, vido_dis_flow + Verify.*:   " + " ".join("%.4f" % e for e in err_ver))
    lines.append("Verify.Descriptor (MaxHamming %d): %d static points checked, %d rejected (%.3f); Verify.ObjectPatch: %d object points checked, %d rejected (%.3f), %d without texture" % (
        MAX_HAMMING, rej["desc"][0], rej["desc"][1], rej["desc"][1] / max(rej["desc"][0], 1), rej["patch"][0], rej["patch"][1], rej["patch"][1] / max(rej["patch"][0], 1), rej["patch"][2]))
    lines.append("condition: translation error <= %.2f m at every frame with vido_dis_flow: max %.4f m -> %s" % (MAX_TRANSLATION_ERROR, max(err_dis), "met" if max(err_dis) <= MAX_TRANSLATION_ERROR else "MISSED"))
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r20"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r20", "dis_tracker_gpu.txt"), "w") as fh:
            fh.write("tests/test_dis_pipeline_gpu.py::test_tracker_on_the_ops_flow — Scene3D(seed 3, one object), 12 frames, 640 x 480, MI355X\n" + "\n".join(lines) + "\n")
    except OSError:
        pass                                                                      # (a read-only tree: the figures are printed above)
    assert max(err_dis) <= MAX_TRANSLATION_ERROR, err_dis
