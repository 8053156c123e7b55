"""GPU: network-node rewrites (nets/fuse.py: folded batch norms + fused epilogue, hipGraph replay) against the plain module graphs, and the
pipelined chain nets -> hand-over -> System::TrackRGBD (pipeline.NetNodes / EndToEnd)."""
import os
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def test_folded_batchnorm_equals_plain_graph(vido):
    from vido_slam_amd import nets
    ctx = vido.Context(width=640, height=480, max_batch=1)
    ops = nets.HipOps(ctx)
    cfg = nets.MaskRCNNConfig(blocks=(3, 4, 6, 3), groups=4, width_per_group=4, res2_out=32, stem_out=16, fpn_out=16, mlp_dim=64, num_classes=7,
                              mask_layers=(16, 16, 16, 16), detections_per_img=20)
    net = nets.fill_maskrcnn(nets.MaskRCNN(ops, cfg), 3).eval().cuda()
    x = torch.rand(1, 3, 160, 224, device="cuda") * 255
    with torch.no_grad():
        ref = net.backbone(x)
        n = nets.fold_batchnorm(net, ops)
        assert n == 16 * 3 + 4 + 1                                   # 16 bottlenecks x 3 + 4 downsample branches + stem
        out = net.backbone(x)
    for a, b in zip(out, ref):
        assert rel_err(a, b) < 1e-4
    md = nets.fill_deterministic(nets.MonoDepth2(), 2).eval().cuda()
    img = torch.rand(1, 3, 192, 640, device="cuda")
    with torch.no_grad():
        ref = md(img)
        assert nets.fold_batchnorm(md, ops) == 20                    # ResNet-18: conv1 + 8 blocks x 2 + 3 downsample branches
        out = md(img)
    assert rel_err(out, ref) < 1e-4                     # folding moves the scale inside the fp32 accumulation: rounding-level differences through 20 layers


def test_graph_replay_equals_eager(vido):
    from vido_slam_amd import nets
    ctx = vido.Context(width=640, height=480, max_batch=1)
    ops = nets.HipOps(ctx)
    lfn = nets.fill_deterministic(nets.LiteFlowNet(ops.correlation, epilogue=ops.bias_act_), 1).eval().cuda()
    rng = np.random.RandomState(0)
    a = torch.as_tensor((rng.rand(128, 192, 3) * 255).astype(np.uint8), device="cuda"); b = torch.as_tensor((rng.rand(128, 192, 3) * 255).astype(np.uint8), device="cuda")
    fn = lambda p, q: nets.analyse_flow(lfn, p, q)
    ref = fn(a, b).clone()
    g = nets.Graphed(fn, [a, b])
    out = g(a, b)
    torch.cuda.synchronize()
    assert rel_err(out, ref) < 2e-5                                # (MIOpen's split-K convolutions are not bit-reproducible from call to call)
    out2 = g(b, a).clone(); torch.cuda.synchronize()
    assert rel_err(out2, fn(b, a)) < 2e-5                          # new inputs flow through the static buffers


def test_pipelined_chain_tracks_and_hands_over(tmp_path, vido):
    """EndToEnd on a short clip, 160x... no: full 640x480 (the facade's ORB grid needs it), full-size nets."""
    from vido_slam_amd import pipeline, synth
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    n = 6
    scene = synth.convoy_scene(n + 1)
    net_ctx = vido.Context(width=640, height=480, max_batch=1)
    nodes = pipeline.NetNodes(net_ctx, 480, 640)
    assert nodes.folded > 100
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    for k in range(n):
        g, d, f, m = scene.frame(k)
        e2e.push(synth.gray_to_bgr(g), (np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)))
    e2e.finish()
    assert len(e2e.poses) == n
    for k, T in enumerate(e2e.poses):
        E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
        assert np.linalg.norm(E[:3, 3]) < 0.05, (k, E)
    assert e2e.stats[-1]["n_objects"] >= 4                          # the five convoy objects are tracked as dynamic
    # the network hand-over ring was filled on the device (flow of the last frame: finite numbers, mask u8 range, depth MONO16 range), the detector ran as one graph
    db = e2e.dev[(n - 1) % e2e.RING]
    assert bool(torch.isfinite(db["flow"]).all()) and float(db["depth"].max()) <= 65535 and int(db["mask"].min()) >= 0
    assert nodes.g_det is not None and nodes.det_overflows == 0 and 0 < e2e.n_det[-1] <= 100
    poses_dev = [T.copy() for T in e2e.poses]
    e2e.close(); slam.close()
    # the same clip through round 2's hand-over (maps to pinned host buffers, TrackRGBD uploads them again): the device-resident hand-over changes where the maps live,
    # not what the tracker computes
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given", handover="host")
    for k in range(n):
        g, d, f, m = scene.frame(k)
        e2e.push(synth.gray_to_bgr(g), (np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)))
    e2e.finish()
    for a, b in zip(poses_dev, e2e.poses):
        assert np.array_equal(a, b)
    e2e.close(); slam.close()


def test_static_detector_head_equals_the_dynamic_one(vido):
    """nets/maskrcnn.py::heads_static / analyse_image_static (fixed shapes, no host synchronisation, one hipGraph with the trunk) against heads() / analyse_image (the
    reference's data-dependent flow, validated stage by stage against the reference fixture in test_maskrcnn_gpu.py) on the SAME trunk outputs of the full-size detector:
    same detections in the same order, same masks, same label image."""
    from vido_slam_amd import pipeline, synth, nets
    net_ctx = vido.Context(width=640, height=480, max_batch=1)
    nodes = pipeline.NetNodes(net_ctx, 480, 640)
    net = nodes.mask_net
    scene = synth.convoy_scene(3)
    for k in range(2):
        bgr = torch.as_tensor(synth.gray_to_bgr(scene.frame(k)[0]), device="cuda")
        with torch.no_grad():
            feats, logits, deltas = [[t.clone() for t in ts] for ts in nodes.g_trunk(bgr)]      # (copies: analyse_image below replays the trunk graph into the same static tensors,
            #                                                                                     and the library GEMMs are not bit-reproducible from replay to replay)
            dyn = net.heads(feats, logits, deltas, nodes.mask_feed)
            sta = net.heads_static(feats, logits, deltas, nodes.mask_feed)
            n = int(sta["n_det"])
            assert n == len(dyn["boxes"]) and 0 < n <= 100
            assert torch.equal(sta["labels"][:n], dyn["labels"]) and torch.equal(sta["scores"][:n], dyn["scores"]) and torch.equal(sta["boxes"][:n], dyn["boxes"])
            # the mask head sees batch 100 instead of a bucket: its four 3x3 layers take different kernels (direct split-fp16 with 16-row or 8-row blocks, Winograd below 128
            # workgroups), the tail computes one class channel with float64 sums instead of 81 with fp32: probabilities equal to 1.5e-4 (measured: 1.0e-4 .. 1.5e-4 box to box;
            # they are thresholded at 0.5 — the label images below differ in isolated pixels only).  Kept at 5e-4, not 1e-4: against a float64 evaluation of the mask head on
            # the same pooled features the static head is 4.1e-4 off, the dynamic one 4.4e-4 and the plain fp32 library chain 3.9e-4 (tests/test_fullsize_gpu.py::
            # test_mask_head_against_float64) — the fp32 rounding of large, cancelling logits, not the split-fp16 kernels — so 1e-4 would sit below the measured 1.5e-4
            assert float((sta["masks"][:n] - dyn["masks"]).abs().max()) < 5e-4
            assert bool((sta["labels"][n:] == 0).all()) and bool((sta["boxes"][n:] == 0).all())
            img_s, lab_s, n_lab, n_det = nets.analyse_image_static(net, feats, logits, deltas, (480, 640), feed=nodes.mask_feed, confidence=nodes.confidence)
            img_d, lab_d = nets.analyse_image(net, bgr, feed=nodes.mask_feed, confidence=nodes.confidence, trunk=nodes.g_trunk)
            assert int(n_det) == n and int(n_lab) == len(lab_d)
            assert sorted(lab_s[:int(n_lab)].tolist()) == sorted(lab_d.tolist()) and bool((lab_s[int(n_lab):] == 0).all())
            assert float((img_s != img_d).float().mean()) < 1e-3                                    # isolated pixels at the 0.5 threshold of the pasted masks
            # the torch-op form of the static head (round 3's first version; the default runs the selection logic in csrc/detpost.hip): identical slots
            net.fused_post = False
            st2 = net.heads_static(feats, logits, deltas, nodes.mask_feed)
            net.fused_post = True
            # (the selection kernels themselves are compared bit for bit on synthetic, tie-heavy inputs in test_maskrcnn_gpu.py; here the two heads each run the box head's
            #  GEMMs, which are not bit-reproducible from call to call)
            assert torch.equal(st2["proposals"], sta["proposals"]) and torch.equal(st2["objectness"], sta["objectness"])
            assert int(st2["n_det"]) == n and torch.equal(st2["labels"], sta["labels"])
            assert float((st2["scores"] - sta["scores"]).abs().max()) < 1e-5 and float((st2["boxes"] - sta["boxes"]).abs().max()) < 1e-2
            # and the captured graph returns the same as the eager static head
            mask_g, lab_g, n_lab_g, n_det_g = nodes.g_det(bgr)
            assert int(n_det_g) == n and float((mask_g.to(torch.uint8) != img_s).float().mean()) < 1e-3


def test_feed_nets_hand_over_contract_at_full_size(vido, oracle):
    """BASELINE configs[2] -> configs[1] with the networks' OWN outputs (bench.py --feed nets), 10 frames, deterministic weights, full-size nodes (LiteFlowNet at 640x480 with
    its half-resolution flow upsampled, MonoDepth2's MONO16 disparity image, Mask R-CNN's u8 label image): the tracker's front end on the device-resident maps
    (vido_frontend_batch through NetNodes' graphs) against the oracle fed the same maps — keypoints, descriptors, static candidates and dense object samples bit-exact."""
    from vido_slam_amd import pipeline, synth
    W, H = 640, 480
    net_ctx = vido.Context(width=W, height=H, max_batch=1)
    nodes = pipeline.NetNodes(net_ctx, H, W)
    ctx = vido.Context(width=W, height=H, max_batch=1)
    p = vido.track_params(dataset=2, depth_map_factor=256.0, bf=387.57, kaist_scale=1.2, th_depth_bg=80.0, th_depth_obj=60.0)      # MONO16 disparity -> metres like the KAIST settings
    ff = vido.FrameFeatures(ctx, p)
    op = oracle.orb_params(n_features=2000, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7)
    scene = synth.convoy_scene(12)
    prev = None; seen_obj = 0
    for k in range(11):
        bgr_h = synth.gray_to_bgr(scene.frame(k)[0])
        cur = torch.as_tensor(bgr_h, device="cuda")
        if prev is None:
            prev = cur; continue
        flow, depth, mask, labels, evs = nodes.infer(prev, cur)
        flow, depth, mask = flow.clone(), depth.clone(), mask.clone()
        torch.cuda.synchronize()
        assert flow.shape == (H, W, 2) and depth.dtype == torch.float32 and float(depth.max()) <= 65535 and mask.dtype == torch.int32 and int(mask.max()) <= 255
        fh, dh, mh = flow.cpu().numpy(), depth.cpu().numpy(), mask.cpu().numpy()
        gray = pipeline.bgr_to_gray(cur)
        torch.cuda.synchronize()                                     # the front end runs on its context's own stream
        out = ff.frontend_batch(k & 1, (gray.data_ptr(), 1, H, W, H * W, W), depth.data_ptr(), flow.data_ptr(), mask.data_ptr(), alias=True)
        n_kp, n_stat, n_obj = int(out["n_kp"][0]), int(out["n_stat"][0]), int(out["n_obj"][0])
        g = oracle.bgr2gray(bgr_h)
        assert np.array_equal(g, gray.cpu().numpy())
        rk, rd, _ = oracle.orb_extract(op, g)
        assert n_kp == len(rk) and n_kp > 500
        kp = np.array(out["kps"][0])[:n_kp]
        for f in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(kp[f], rk[f]), (k, f)
        assert np.array_equal(np.array(out["desc"][0])[:n_kp], rd)
        dref = oracle.depth_prescale(dh.copy(), 2, p.depth_map_factor, p.bf, p.kaist_scale)
        i, c, fl, dd = oracle.static_candidates(rk, dref, fh, mh, p.th_depth_bg)
        assert n_stat == len(i)
        assert np.array_equal(np.array(out["stat_idx"][0])[:n_stat], i) and np.array_equal(np.array(out["stat_corr"][0])[:n_stat], c)
        assert np.array_equal(np.array(out["stat_flow"][0])[:n_stat], fl) and np.array_equal(np.array(out["stat_depth"][0])[:n_stat], dd)
        kk, cc, od, lab, ofl = oracle.dense_object_samples(dref, fh, mh, p.th_depth_obj)
        assert n_obj == len(kk)
        assert np.array_equal(np.array(out["obj_keys"][0])[:n_obj], kk) and np.array_equal(np.array(out["obj_label"][0])[:n_obj], lab)
        assert np.array_equal(np.array(out["obj_depth"][0])[:n_obj], od) and np.array_equal(np.array(out["obj_flow"][0])[:n_obj], ofl)
        seen_obj += n_obj
        prev = cur


def test_two_chain_schedule_returns_the_same_maps(vido):
    """NetNodes(streams="flow+depth") — LiteFlowNet + MonoDepth2 on a side stream next to the detector, the default — against everything on the caller's stream: same flow,
    depth and label image once the returned events have fired (the graphs are the same; only the queues differ)."""
    from vido_slam_amd import pipeline, synth
    scene = synth.convoy_scene(4)
    fr = [torch.as_tensor(synth.gray_to_bgr(scene.frame(k)[0]), device="cuda") for k in range(3)]
    outs = []
    for mode in ("flow+depth", False):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, streams=mode)
        assert (nodes.streams is not None) == bool(mode)
        res = []
        for k in (1, 2):
            flow, depth, mask, labels, evs = nodes.infer(fr[k - 1], fr[k])
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            res.append((flow.clone(), depth.clone(), mask.clone()))
        torch.cuda.synchronize(); outs.append(res)
    for (fa, da, ma), (fb, db, mb) in zip(*outs):
        assert float((fa - fb).abs().max()) < 1e-3 and float((da.float() - db.float()).abs().max()) <= 2.0      # (library GEMMs are not bit-reproducible; depth is a 16-bit integer scale)
        assert float((ma != mb).float().mean()) < 1e-3


def test_bench_two_ranks_on_one_gpu_prints_the_n2_line():
    """`python bench.py --gpus 2 --oversubscribe --full`: the self-spawn through torch.distributed.run (the driver's launcher), two ranks (both on GPU 0, gloo), the replicated
    per-frame chain with barrier + max-over-ranks timing, the landmark-sharded global BA with an all-reduce per LM trial, ONE JSON line from rank 0 with n_gpus = 2.
    The numbers mean nothing on one GPU; the point is that the N > 1 path has executed end to end before a multi-GPU node runs it (round-3 review, item 3c)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--oversubscribe", "--steps", "3", "--warmup", "1", "--prologue", "3", "--cpu-baseline", "0",
           "--gba-cams", "80", "--gba-points", "6000", "--full"]
    env = dict(os.environ); env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                        # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["value"] > 0
    g = d["extra"]["global_ba"]
    assert g["n_gpus"] == 2 and "gloo" in g["collective"] and g["lm_iterations"] >= 1 and g["chi2"][1] < g["chi2"][0]
    assert d["global_ba_iters_per_s"]["n_gpus"] == 2


def test_plain_bench_run_prints_the_headline_alone(tmp_path):
    """`python bench.py` without --full: the headline chain, its stage breakdown and --dump-outputs, and none of the side measurements (each of those is a run of
    its own behind --full)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--prologue", "3", "--dump-outputs", str(tmp_path / "dump")]
    env = dict(os.environ); env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 0.01 * d["ms_per_step"] + 0.01
    assert d["stage_ms"]["track_total_ms"] > 0 and d["per_frame_counts"]["keypoints"] > 0
    assert not {"extra", "roofline", "roofline_nets", "cpu_baseline", "global_ba_iters_per_s"} & set(d), sorted(d)
    assert {"flow", "depth", "mask", "pose_Tcw"} <= {f[:-4] for f in os.listdir(tmp_path / "dump")}
