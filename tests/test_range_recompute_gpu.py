"""Recovery from split-fp16 range overflow: the per-frame latch (vido_range_latch / HipOps.range_latch), the range-safe scope (nets.range_safe: every split-fp16 entry
point declines, the callers' fp32 routes run), NetNodes(on_range="recompute") with infer_checked / recompute, EndToEnd's per-frame words, and the standalone node functions'
on_range argument.

The trigger.  The image-facing convolution of LiteFlowNet (netFeatures.netOne.0) and of the detector (the stem) get non-negative weights, scaled: the layers then answer the
frame's BRIGHTNESS, and the activations behind them grow with it.  A dark frame (values 0 .. 50) stays inside fp16's range everywhere, a bright one (200 .. 255) leaves it in
both networks.  Measured with the plain fp32 modules on the host (largest |input| over all convolution / linear layers but the first): LiteFlowNet at scale 300 — dark pair
2.2e4, (dark, bright) pair 2.6e5 (a 64-channel 3x3 layer of the finest level, on the direct split-fp16 kernel: 2.4e5); the detector at 0.7 — dark 2.4e4, bright 1.8e5 (the RPN
head's 3x3 at P2: 1.4e5, layer4's last 1x1: 1.1e5).  LiteFlowNet sees the bright frame in two pairs: (previous, bright) and (bright, next) both trip its context."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F = torch.nn.functional
LFN_SCALE, DET_SCALE = 300.0, 0.7
TOL = 1e-3                                                   # tests/test_fullsize_gpu.py
OFF = ("VIDO_NO_WINO", "VIDO_NO_CONV1X1", "VIDO_NO_CONVSMALL", "VIDO_NO_CONVDIRECT", "VIDO_NO_GCONV", "VIDO_NO_GCONV_S2", "VIDO_NO_DEPTH_FUSED")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def brighten(net):
    """the trigger (module docstring), in place, before the network meets a device or a graph"""
    from vido_slam_amd import nets
    with torch.no_grad():
        if isinstance(net, nets.LiteFlowNet):
            net.netFeatures.netOne[0].weight.abs_().mul_(LFN_SCALE)
        elif isinstance(net, nets.MaskRCNN):
            net.backbone.body.stem.conv1.weight.abs_().mul_(DET_SCALE)
    return net


def patch_fills(monkeypatch):
    from vido_slam_amd import nets
    fd, fm = nets.fill_deterministic, nets.fill_maskrcnn
    monkeypatch.setattr(nets, "fill_deterministic", lambda net, seed: brighten(fd(net, seed)))
    monkeypatch.setattr(nets, "fill_maskrcnn", lambda net, seed: brighten(fm(net, seed)))


def scene_frames(n):
    """(BGR frames dark / bright on demand, given maps): the convoy scene of tests/test_e2e_gpu.py, its gray images mapped to 0 .. 50 (dark) or 200 .. 255 (bright)"""
    from vido_slam_amd import synth
    scene = synth.convoy_scene(n + 1)
    out = []
    for k in range(n):
        g, d, f, m = scene.frame(k)
        g = g.astype(np.float32) / 255.0
        out.append(dict(dark=synth.gray_to_bgr((50 * g).astype(np.uint8)), bright=synth.gray_to_bgr((200 + 55 * g).astype(np.uint8)),
                        given=(np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32))))
    return scene, out


@pytest.fixture(scope="module")
def rig(vido):
    from vido_slam_amd import pipeline
    mp = pytest.MonkeyPatch()
    patch_fills(mp)
    ctx = vido.Context(width=640, height=480, max_batch=1)
    try:
        nodes = pipeline.NetNodes(ctx, 480, 640, on_range="recompute", calibrate_scores=False)    # (calibration would meet a mid-grey frame with the trigger in place)
    finally:
        mp.undo()
    assert nodes.graph_error is None and nodes.g_flow is not None and nodes.g_trunk is not None and nodes.g_det is not None, nodes.graph_error
    scene, fr = scene_frames(5)
    dev = lambda a: torch.as_tensor(a).cuda()
    frames = [dict(dark=dev(x["dark"]), bright=dev(x["bright"]), given=x["given"]) for x in fr]
    torch.cuda.synchronize()
    nodes.ops.conv1x1_range_flag(reset=True); nodes.ops_flow.conv1x1_range_flag(reset=True)      # (construction: warm-up frames)
    yield nodes, scene, frames
    ctx.close()


def test_latch_attributes_trips_to_the_launches_before_it(vido):
    """On each of two contexts: a conv3x3_h launch with one activation at 1e5, latch into A, a clean launch, latch into B -> A = 1, B = 0 and the live flag 0; a device
    word works as well as a pinned one, and a latch ORs (it never clears a word)."""
    from vido_slam_amd.nets.ops import HipOps, pack_conv3x3_h
    ctxs = [vido.Context(), vido.Context()]
    try:
        w = pack_conv3x3_h(torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(1))).cuda()
        for c in ctxs:
            ops = HipOps(c)
            ops.conv1x1_range_flag(reset=True)
            for where in ("pinned", "device"):
                A = torch.zeros(1, dtype=torch.int32); B = torch.zeros(1, dtype=torch.int32)
                A, B = (A.pin_memory(), B.pin_memory()) if where == "pinned" else (A.cuda(), B.cuda())
                x = torch.randn(1, 64, 16, 16, device="cuda"); x[0, 5, 7, 7] = 1e5
                ops.conv3x3_h_bias_act(x, w, None, 64, 1.0)
                ops.range_latch(A)
                ops.conv3x3_h_bias_act(torch.randn(1, 64, 16, 16, device="cuda"), w, None, 64, 1.0)
                ops.range_latch(B)
                torch.cuda.synchronize()
                assert (int(A[0]), int(B[0]), ops.conv1x1_range_flag(reset=False)) == (1, 0, 0), (where, int(A[0]), int(B[0]))
                ops.range_latch(A); torch.cuda.synchronize()
                assert int(A[0]) == 1                                 # nothing tripped since: the word keeps its bit
    finally:
        for c in ctxs:
            c.close()


def _hostile(kind, shape, seed):
    """case (a) of tests/test_split_fp16_gpu.py with a few activations at up to 1e6 (past fp16's 65504)"""
    from test_split_fp16_gpu import make_case
    x, w, b, r, slope = make_case(kind, shape, "a", seed)
    g = torch.Generator().manual_seed(seed + 1)
    flat = x.view(-1)
    idx = torch.randint(0, flat.numel(), (16,), generator=g)
    flat[idx] = torch.rand(16, generator=g) * 9e5 + 1e5
    return x, w, b, slope


@pytest.mark.parametrize("kind", ["c1", "c3", "fc", "dc"])
def test_range_safe_route(vido, kind):
    """The four split-fp16 entry points on activations up to 1e6: with the default ops the split kernel runs and the flag rises; inside nets.range_safe(ops) the entry point
    declines (1x1, fully connected, transposed: None -> the caller's library route) or takes fp32 Winograd (3x3), the flag stays 0, the outputs are finite and within
    tests/test_split_fp16_gpu.py's elementwise bound against float64 (the 3x3: bit-identical to the fp32 Winograd kernel, whose error is that kernel's own)."""
    from vido_slam_amd import nets
    from vido_slam_amd.nets.ops import HipOps, pack_wino3x3
    from test_split_fp16_gpu import reference
    ctx = vido.Context()
    try:
        ops = HipOps(ctx); ops.conv1x1_range_flag(reset=True)
        shape = {"c1": (256, 256, 100, 68), "c3": (1, 256, 256, 100, 136), "fc": (333, 2048, 256), "dc": (3, 64, 128, 6, 10)}[kind]
        x, w, b, slope = _hostile(kind, shape, 11)
        xc, bc = x.cuda(), b.cuda()
        if kind == "fc":
            mod = torch.nn.Linear(w.shape[1], w.shape[0]).cuda()
        elif kind == "dc":
            mod = torch.nn.ConvTranspose2d(w.shape[0], w.shape[1], 2, 2).cuda()
        else:
            mod = torch.nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], 1, w.shape[2] // 2).cuda()
        with torch.no_grad():
            mod.weight.copy_(w); mod.bias.copy_(bc)
        call = {"c1": lambda: ops.conv1x1_conv(mod, xc, slope), "c3": lambda: ops.wino3x3_conv(mod, xc, slope), "fc": lambda: ops.fc_h_linear(mod, xc, slope),
                "dc": lambda: ops.deconv2x2_conv(mod, xc, slope)}[kind]
        with torch.no_grad():
            y = call(); torch.cuda.synchronize()
            assert y is not None and ops.conv1x1_range_flag(reset=True) == 1, kind          # the split-fp16 kernel ran and saw the range left
            with nets.range_safe(ops) as held:
                assert held == [ops] and ops.range_safe_active
                y = call()
            assert not ops.range_safe_active
            if kind == "c3":
                form = ops.wino3x3_form(*x.shape[:2], w.shape[0], *x.shape[2:])
                yw = ops.wino3x3_bias_act(xc.contiguous(), pack_wino3x3(w, form).cuda(), bc, int(w.shape[0]), slope, form)
                assert y is not None and torch.equal(y, yw)
            else:
                assert y is None, kind                                # declined: the callers' fp32 routes
                y = {"c1": lambda: F.leaky_relu(mod(xc), slope), "fc": lambda: F.leaky_relu(mod(xc), slope), "dc": lambda: F.leaky_relu(mod(xc), slope)}[kind]()
            torch.cuda.synchronize()
        assert ops.conv1x1_range_flag(reset=True) == 0, kind
        assert bool(torch.isfinite(y).all()), kind
        K = {"c1": shape[0], "c3": 9 * shape[1], "fc": shape[1], "dc": shape[1]}[kind]
        y64, bound = reference(kind, x, w, b, None, slope, K)
        q = float(((y.cpu().double() - y64).abs() / bound.clamp_min(1e-300)).max())
        print("range_safe %s: max |y - y64| / bound %.3f, relative to the output's scale %.2e" % (kind, q, rel(y.cpu(), y64)))
        if kind == "c3":
            assert rel(y.cpu(), y64) < 1e-5, rel(y.cpu(), y64)            # (Winograd's transforms amplify rounding past an FMA-chain envelope — as MIOpen's default 3x3
        else:                                                             #  algorithm does, tests/test_split_fp16_gpu.py — so the 3x3 is held to its scale)
            assert q <= 1.0, (kind, q)
    finally:
        ctx.close()


def test_range_safe_scope_on_modules_and_the_bottleneck(vido, rig):
    """nets.range_safe(module) finds the HipOps a network launches through (the detector's, LiteFlowNet's), and inside it the detector's trunk — fused bottlenecks, FPN
    laterals, direct 3x3 layers — runs without one split-fp16 launch even on a bright frame."""
    from vido_slam_amd import nets
    nodes, _, frames = rig
    with nets.range_safe(nodes.mask_net) as held:
        assert nodes.ops in held
        with nets.range_safe(nodes.flow_net) as held2:
            assert nodes.ops_flow in held2
        nodes._trunk_fn(frames[2]["bright"])
    torch.cuda.synchronize()
    assert nodes.ops.conv1x1_range_flag(reset=True) == 0
    nodes._trunk_fn(frames[2]["bright"]); torch.cuda.synchronize()
    assert nodes.ops.conv1x1_range_flag(reset=True) == 1                  # the same call outside the scope: the trigger is real


def _snapshot(nodes, prev, cur):
    f = nodes.g_flow(prev, cur).clone()
    t = [a.clone() for grp in nodes.g_trunk(cur) for a in grp]
    d = [a.clone() for a in nodes.g_det(cur)]
    torch.cuda.synchronize()
    return [f] + t + d


def test_graphs_untouched_by_a_recompute(vido, rig):
    """Replays of g_flow, g_trunk and g_det on a frame A, a forced recomputation of both networks on another frame, replays on A again: bit-identical (the scope never
    replaces or frees a packed weight a graph reads)."""
    nodes, _, frames = rig
    A0, A1, B = frames[0]["dark"], frames[1]["dark"], frames[2]["bright"]
    ref = _snapshot(nodes, A0, A1); ref2 = _snapshot(nodes, A0, A1)       # (the library's split-K kernels: replay-to-replay spread, if any)
    keep = {id(m): (getattr(m, "_c1_w", None), getattr(m, "_c3h_w", None)) for m in list(nodes.mask_net.modules()) + list(nodes.flow_net.modules())}
    n0 = dict(nodes.range_recomputes)
    nodes.recompute(A1, B, flow=True, detector=True); torch.cuda.synchronize()
    assert nodes.range_recomputes == {"flow": n0["flow"] + 1, "detector": n0["detector"] + 1}
    for m in list(nodes.mask_net.modules()) + list(nodes.flow_net.modules()):
        a, b = keep[id(m)]
        assert getattr(m, "_c1_w", None) is a and getattr(m, "_c3h_w", None) is b
    got = _snapshot(nodes, A0, A1)
    for i, (a, r1, r2) in enumerate(zip(got, ref, ref2)):
        if a.is_floating_point():
            spread = rel(r2, r1)
            assert rel(a, r1) <= 2.0 * spread + 1e-7, (i, rel(a, r1), spread)       # bit-identical where replays are; within their own spread elsewhere
        else:
            assert torch.equal(a, r1) or torch.equal(a, r2), i
    nodes.ops.conv1x1_range_flag(reset=True); nodes.ops_flow.conv1x1_range_flag(reset=True)


def _plain(nodes, monkeypatch):
    """the plain eager fp32 modules with the same (triggered) weights and every switch off (tests/test_fullsize_gpu.py)"""
    from vido_slam_amd import nets
    from vido_slam_amd.nets.ops import correlation_torch_reference
    for k in OFF + ("VIDO_NO_FC_H", "VIDO_NO_DECONV_H"):
        monkeypatch.setenv(k, "1")
    lfn = brighten(nets.fill_deterministic(nets.LiteFlowNet(correlation_torch_reference), 1)).eval().cuda()
    det = brighten(nets.fill_maskrcnn(nets.MaskRCNN(nodes.ops), 1 + 2)).eval().cuda()
    return lfn, det


def test_trigger_and_infer_checked_recompute(vido, rig, monkeypatch):
    """The trigger is real: in the default mode (on_range="raise") the bright frame raises and the dark one does not.  With on_range="recompute", infer_checked on the bright
    frame recomputes each network once and returns finite maps within tests/test_fullsize_gpu.py's tolerances of the plain eager fp32 modules (same weights)."""
    nodes, _, frames = rig
    dark0, dark1, bright = frames[0]["dark"], frames[1]["dark"], frames[2]["bright"]
    nodes.on_range = "raise"
    try:
        nodes.infer_checked(dark0, dark1)
        with pytest.raises(RuntimeError) as e:
            nodes.infer_checked(dark1, bright)
        assert "flow" in str(e.value) and "detector" in str(e.value) and "recompute" in str(e.value)
        nodes.infer(dark1, bright); torch.cuda.synchronize()          # (the old check sees it too)
        with pytest.raises(RuntimeError):
            nodes.check_conv1x1_range()
    finally:
        nodes.on_range = "recompute"
    n0 = dict(nodes.range_recomputes)
    flow, depth, mask, labels, evs = nodes.infer_checked(dark1, bright)
    assert nodes.range_recomputes == {"flow": n0["flow"] + 1, "detector": n0["detector"] + 1}
    n_lab, n_det = (int(v) for v in nodes.last_counts)
    r = nodes.redo_detector_if_overflowed(bright, n_det, range_safe=True)      # (saturated scores: the static head's slots may not hold every detection)
    if r is not None:
        mask, labels = r; n_lab = len(labels)
    flow, mask = flow.clone(), mask.clone(); labels = labels[:n_lab].clone()
    torch.cuda.synchronize()
    assert nodes.ops.conv1x1_range_flag(reset=False) == 0 and nodes.ops_flow.conv1x1_range_flag(reset=False) == 0
    assert bool(torch.isfinite(flow).all()) and bool(torch.isfinite(depth).all())
    lfn, det = _plain(nodes, monkeypatch)
    from vido_slam_amd import nets
    with torch.no_grad():
        ref = nets.analyse_flow(lfn, dark1, bright)
        img_p, labels_p = nets.analyse_image(det, bright, feed=nodes.mask_feed, confidence=nodes.confidence)
    # LiteFlowNet's flow at this trigger is 1e5 px: its warps sample outside the image, and two correct fp32 routes differ in the leading digit (measured 1.2 relative) — the
    # flow is held to finite values, and the recomputation's arithmetic to the feature pyramid both images go through (no warp), against the plain module
    x = bright.flip(-1).permute(2, 0, 1).float().div(255.0).unsqueeze(0) - nodes.flow_net._mean_second
    with torch.no_grad():
        with nets.range_safe(nodes.flow_net):
            fa = nodes.flow_net.netFeatures(x)
        fr = lfn.netFeatures(x)
        fh = nodes.flow_net.netFeatures(x); torch.cuda.synchronize()
    nodes.ops_flow.conv1x1_range_flag(reset=True)
    e = max(rel(a, b) for a, b in zip(fa, fr))
    agree = float((mask.to(torch.int32) == img_p.to(torch.int32)).float().mean())
    print("recomputed bright frame: feature pyramid relative error %.2e (scale %.3g), flow scale %.3g, %d labels, label image agreement %.5f"
          % (e, max(float(b.abs().max()) for b in fr), float(ref.abs().max()), n_lab, agree))
    assert e < TOL, e
    assert sorted(int(v) for v in labels.tolist()) == sorted(int(v) for v in labels_p.tolist())
    assert agree > 0.999, agree


def test_end_to_end_recomputes_the_bright_frame(vido, rig, tmp_path):
    """EndToEnd (feed="given") on dark, dark, bright, dark, dark: every frame tracked without error; frame 2 recomputed in both networks, frame 3 in LiteFlowNet (its pair
    holds the bright frame), nothing else; the parked maps the recomputation did not touch are bit-identical to graph replays of the same inputs."""
    from vido_slam_amd import pipeline
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    nodes, scene, frames = rig
    kinds = ["dark", "dark", "bright", "dark", "dark"]
    n0 = dict(nodes.range_recomputes)
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    parked = []
    try:
        for k, kind in enumerate(kinds):
            e2e.push(frames[k][kind].cpu().numpy(), frames[k]["given"])
            e2e.finish()                                          # (the frame tracked: its slot is read before the ring wraps)
            db = e2e.dev[k % e2e.RING]
            parked.append((db["flow"].clone(), db["depth"].clone(), db["mask"].clone()))
        e2e.finish()
    finally:
        e2e.close()
    assert e2e.err is None and len(e2e.poses) == len(kinds) == len(e2e.stats)
    assert e2e.range_frames == [2, 3], e2e.range_frames
    assert nodes.range_recomputes == {"flow": n0["flow"] + 2, "detector": n0["detector"] + 1}, nodes.range_recomputes
    for k, kind in enumerate(kinds):
        cur = frames[k][kind]; prev = frames[k - 1][kinds[k - 1]] if k else cur
        f = nodes.g_flow(prev, cur).clone(); d = nodes.g_depth(cur).clone()
        m, _, _, n_det = nodes.g_det(cur); m = m.clone(); n_det = int(n_det)
        if n_det > nodes.mask_net.config.detections_per_img:          # (EndToEnd's overflow redo: the dynamic head after the trunk's graph)
            m = nodes.redo_detector_if_overflowed(cur, n_det)[0]
        torch.cuda.synchronize()
        # (graph replays are not bit-reproducible where a library kernel's summation order varies from launch to launch: tests/test_fullsize_gpu.py, test_e2e_gpu.py bounds)
        assert float((parked[k][1] - d).abs().max()) <= 64.0, k       # MonoDepth2 is never recomputed (MONO16 counts)
        # (the triggered LiteFlowNet is chaotic — two eager calls on the same dark pair differ in the leading digit, see test_trigger_and_infer_checked_recompute —
        # so its flow is held to finite values; which frames it was recomputed on is range_frames / range_recomputes above)
        assert bool(torch.isfinite(parked[k][0]).all()), k
        if k not in (2, 3):
            assert bool(torch.isfinite(f).all()), k
        else:
            assert not bool(torch.isfinite(f).all()), k                # (the graph's split-fp16 route on these pairs: what the recomputation replaced)
        if k != 2:
            assert float((parked[k][2] == m).float().mean()) > 0.999, k
    nodes.ops.conv1x1_range_flag(reset=True); nodes.ops_flow.conv1x1_range_flag(reset=True)


def test_standalone_node_functions(vido, rig):
    """analyse_flow / analyse_image with on_range="raise" raise on the bright input; with "recompute" they return finite outputs equal to the range-safe call; with None
    (the default) the result is the unchecked call's."""
    from vido_slam_amd import nets
    nodes, _, frames = rig
    dark, bright = frames[1]["dark"], frames[2]["bright"]
    lfn, det = nodes.flow_net, nodes.mask_net
    kw = dict(feed=nodes.mask_feed, confidence=nodes.confidence)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            nets.analyse_flow(lfn, dark, bright, on_range="raise")
        with pytest.raises(RuntimeError):
            nets.analyse_image(det, bright, on_range="raise", **kw)
        f = nets.analyse_flow(lfn, dark, bright, on_range="recompute")
        with nets.range_safe(lfn):
            fs = nets.analyse_flow(lfn, dark, bright)
        img, lab = nets.analyse_image(det, bright, on_range="recompute", **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(fs).all()) and img.shape == bright.shape[:2]
        assert nodes.ops.conv1x1_range_flag(reset=False) == 0 and nodes.ops_flow.conv1x1_range_flag(reset=False) == 0     # (the repeats ran in fp32's range)
        # None: unchecked (the same call as before this argument existed; the detector: its label image is well-conditioned under the trigger, the flow is not) — and a
        # clean input passes "raise"
        a, la = nets.analyse_image(det, dark, **kw); b, lb = nets.analyse_image(det, dark, on_range=None, **kw); c, lc = nets.analyse_image(det, dark, on_range="raise", **kw)
        assert float((a == b).float().mean()) > 0.999 and float((a == c).float().mean()) > 0.999 and sorted(la.tolist()) == sorted(lb.tolist()) == sorted(lc.tolist())
        assert bool(torch.isfinite(nets.analyse_flow(lfn, dark, frames[0]["dark"], on_range="raise")).all())
        with pytest.raises(ValueError):
            nets.analyse_flow(lfn, dark, dark, on_range="sometimes")
    torch.cuda.synchronize()
    nodes.ops.conv1x1_range_flag(reset=True); nodes.ops_flow.conv1x1_range_flag(reset=True)
