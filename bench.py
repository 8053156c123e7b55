#!/usr/bin/env python3
"""bench.py — driver contract: `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line.

HEADLINE (BASELINE.json metric "frames/sec end-to-end (flow+depth+track+local-BA) at 640x480"): BASELINE configs[1]+[2]+[3] CHAINED on
one GPU, the reference's realtime chain src/realtime_demo/src/run_vido.cc:142-157 (RunNet: FlowNet, MaskRcnn, MonoDepth service calls) ->
:229-235 (System::TrackRGBD).  A step = ONE 640x480 frame through
    LiteFlowNet + MonoDepth2 (fed 640x192) + Mask R-CNN X-101-32x8d-FPN (fed 800x1088), fp32, batch 1        configs[2]
    -> hand-over of flow / depth / mask to the tracker through a device-resident ring (System::TrackRGBDDevice: no map crosses PCIe)
    -> System::TrackRGBD: cvtColor + ORB pyramid/FAST/quadtree/IC-angle/blur/rBRIEF, depth pre-scale, static filter, dense object
       sampling, mask propagation, P3P-RANSAC, PoseOptimizationFlow2Cam, scene flow, object tracking, per-object PoseOptimizationFlow2,
       re-seeding, tracklets                                                                                  configs[1]
    -> PartialBatchOptimization over the 20-frame window (the reference runs it every frame)                  configs[3]
with the two halves PIPELINED like two ROS nodes would be: the networks of frame k+1 run (three hipGraph replays on TWO streams: the detector on the caller's,
LiteFlowNet + MonoDepth2 on one side stream) while frame k is tracked by a worker thread on the tracker's own stream.  The BGR frames are resident in pinned host memory when the timed region starts (the camera's hand-over);
`value` = frames / wall time of the whole chain, max over ranks.  Before the W warm-up steps an untimed prologue of --prologue frames fills
the local-BA window, so every timed frame optimises a full 20-keyframe window.
Synthetic data: a ray-cast 640x480 scene (ground plane, far wall, 5 moving objects, forward-driving camera); the networks have random-init
weights (no checkpoints ship with the reference, no network here), so their outputs carry no geometry: they run at full cost, their
outputs are parked in the device ring, and frame k is tracked only after they have completed, but the tracker is handed the renderer's exact
flow / depth / mask of the same frame (--feed given: uploaded next to the BGR frame; --feed nets hands it the networks' outputs instead — extra.e2e_feed_nets).
Arithmetic: fp32 results everywhere; since round 6 the detector's 1x1 convolutions compute them from 16-bit planes of their fp32 operands — two fp16 planes, three exact
products on the fp16 matrix instruction (the default; VIDO_CONV1X1_ARITH=bf16x3: three bf16 planes, six products) — with fp32 accumulators (config.net_arith;
csrc/conv1x1.hip), with a measured error against float64 below the fp32 instruction's.
The per-frame path does not shard (frame k depends on frame k-1): --gpus N runs N independent replicas, no data-path collective.
--dump-outputs DIR writes what the chain computed for the last timed frame as .npy files (inputs, weights and frames are seeded: the same arguments give the same inputs),
so that two builds can be compared output for output.

A plain run does only what the headline needs: set-up (the frames are rendered on a pool of host threads), prologue, warm-up, the timed steps, --dump-outputs, and the
JSON line with the headline, stage_ms of the timed frames (tracker stages, local BA, the hand-over waits), per_frame_counts, the pose error and the configuration.
--full adds every other measurement below, each a run of its own after the headline (what --no-extra, --cpu-baseline, --batch and --gba-* select applies there).

Extra objects on the same JSON line with --full:
  stage_ms       adds the networks alone (one graph replay each, *_ms) to the per-frame breakdown of the chain
  roofline       dominant hand-written kernel of the tracker front end (FAST): algorithmic bytes / live HIP-event time vs the 8 TB/s HBM peak,
                 measured on BASELINE configs[1] batched (64 frames in flight, the only regime where an HBM roofline of a <1 MB/frame stage means anything)
  roofline_ba    k_ba_linearize at configs[3] (local window) and configs[4] (1 M edges) size: 288 B per edge
  roofline_nets  fp32-EQUIVALENT FLOP/s of each network node vs the 157.3 TFLOP/s fp32 matrix/vector peak (since round 6 the detector's 1x1 / dense 3x3 / FC / transposed layers compute
                 their fp32 results on the 16-bit matrix instructions: its fraction can pass 1)
  roofline_gconv the detector's grouped 3x3 convolution kernel (csrc/gconv.hip) vs the same peak
  roofline_conv3x3 the direct split-fp16 3x3 kernel at the FPN / RPN P2 shape (and the Winograd kernel's time beside it)
  roofline_conv1x1 the split 1x1 GEMM at the detector's layer3 shape: fp32-equivalent TFLOP/s against 2500 / 3 (three fp16 products per multiply-add; / 6 for the bf16 form)
  cpu_baseline   BASELINE.md section 3: the SLAM stages (ORB / lists / pose optimisers / local BA, the C oracle) on ONE pinned core, median and p95 over 50 frames = `value`;
                 the three networks on torch-CPU on all cores as a separate part
  parity_pin     which parts of the oracle are pinned by reference outputs and which are not
  extra          configs[1] batched throughput, per-frame optimisers, Hamming matcher, local / global / dynamic BA, sharded global BA with --gpus N
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: fp32 vector = fp32 matrix peak
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files together


def newest_profile(name):
    """(path relative to the repo, full path) of profiles/rN/<name> for the largest N that has it, or (None, None): every counter the line quotes is READ from a committed
    profile named next to it — nothing is typed in."""
    for n in range(9, 0, -1):
        p = os.path.join(ROOT, "profiles", "r%d" % n, name)
        if os.path.exists(p):
            return "profiles/r%d/%s" % (n, name), p
    return None, None


def read_sq_counters(path, kernel_prefix=None):
    """tools/pmc_fast.sh summary lines: `SQ_INSTS_VALU   4 launches  avg 6.3e+07` -> {counter: mean per launch}"""
    out = {}
    for line in open(path):
        t = line.split()
        if len(t) >= 5 and t[2] == "launches" and t[3] == "avg":
            try:
                out.setdefault(t[0], float(t[4]))
            except ValueError:
                pass
    return out


def write_settings(path, K, w, h):
    """Settings file in the reference's OpenCV-YAML schema (src/config/kitti_config.yaml keys, Tracking.cc:45-171); OMD depth convention (d / factor)."""
    fx, fy, cx, cy = K
    with open(path, "w") as fh:
        fh.write("%%YAML:1.0\nCamera.width: %d\nCamera.height: %d\n" % (w, h))
        fh.write("Camera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.k1: 0.0\nCamera.k2: 0.0\nCamera.p1: 0.0\nCamera.p2: 0.0\nCamera.k3: 0.0\n" % (fx, fy, cx, cy))
        fh.write("Camera.bf: 387.57\nCamera.fps: 30.0\nCamera.RGB: 0\nChooseData: 1\nDepthMapFactor: 1.0\nThDepthBG: 40.0\nThDepthOBJ: 25.0\n")
        fh.write("MaxTrackPointBG: 3000\nMaxTrackPointOBJ: 800\nSFMgThres: 0.12\nSFDsThres: 0.3\nWINDOW_SIZE: 20\nOVERLAP_SIZE: 4\nUseSampleFeature: 0\n")
        fh.write("ORBextractor.nFeatures: 2000\nORBextractor.scaleFactor: 1.2\nORBextractor.nLevels: 8\nORBextractor.iniThFAST: 20\nORBextractor.minThFAST: 7\n")


def dump_outputs(path, arrays):
    """--dump-outputs: every array as path/<name>.npy, float64 where it is float64 and float32 otherwise.  When they would pass DUMP_LIMIT_BYTES together, each
    array of more than 4096 elements is replaced by the same fixed, seeded sample of its flattened elements (sorted indices) in every run with the same shapes."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: v.astype(np.float64 if v.dtype == np.float64 else np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    budget = DUMP_LIMIT_BYTES - (4096 * 8 + 1024) * len(arrays)          # (room for the small arrays and the .npy headers)
    for name, a in arrays.items():
        if total > DUMP_LIMIT_BYTES and a.size > 4096:
            n = max(4096, a.size * budget // total)
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, n, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def _split_pmc(name):
    """traffic_bytes_fetch_x2 of a split-fp16 kernel from the newest profiles/rN/split_kernels_pmc.json (None when there is none)"""
    import glob as _glob, json as _json
    for f in sorted(_glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*", "split_kernels_pmc.json")), reverse=True):
        try:
            return int(_json.load(open(f))["kernels"][name]["traffic_bytes_fetch_x2"])
        except Exception:
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed frames (100 frames = ~2 s: the round-2 review asked for more than 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prologue", type=int, default=20, help="untimed frames before the warm-up that fill the local-BA window (WINDOW_SIZE)")
    ap.add_argument("--feed", choices=("given", "nets"), default="given", help="maps the tracker consumes: the renderer's (default) or the networks' outputs")
    ap.add_argument("--handover", choices=("device", "host"), default="device", help="network -> tracker hand-over: device-resident (default: one BGR upload per frame, no map crosses PCIe) or round 2's pinned-host round trip")
    ap.add_argument("--no-pipeline", action="store_true", help="serial chain: networks of frame k, then tracking of frame k")
    ap.add_argument("--no-graphs", action="store_true"); ap.add_argument("--no-fold", action="store_true"); ap.add_argument("--no-streams", action="store_true", help="(default) the three networks share one stream")
    ap.add_argument("--streams", action="store_true", help="one stream per network (round 3: 69.5 frames/s; round 2 measured this slower than back to back, when the detector head still synchronised the host)")
    ap.add_argument("--net-streams", default="flow+depth", help="which networks leave the main stream: \"flow+depth\" (default: LiteFlowNet and MonoDepth2 share ONE side stream next to the detector: measured 72.5 frames/s against 59.6 with everything back to back), \"none\", \"depth\", \"flow\", \"det\", \"flow,depth\" (one side stream each: 52.7)")
    ap.add_argument("--miopen-find", action="store_true", help="torch.backends.cudnn.benchmark = True (MIOpen measures its solvers once per layer shape)")
    ap.add_argument("--batch", type=int, default=64, help="frames in flight of the configs[1] batched leg")
    ap.add_argument("--cpu-baseline", type=int, default=50, help="frames of the CPU-baseline sample of the SLAM stages on one pinned core (0 = skip; ~0.23 s each)")
    ap.add_argument("--cpu-baseline-net-frames", type=int, default=1, help="frames of the separate torch-CPU sample of the three networks (~10 s each on a 128-thread host)")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--no-extra", action="store_true", help="skip the side measurements (optimisers / BA / matcher)")
    ap.add_argument("--torch-allreduce", action="store_true", help="global BA at N > 1: all-reduce through the torch.distributed hook (two stream synchronisations + a Python call each) instead of "
                                                                   "the default, the library's own ncclAllReduce on its stream (csrc/rccl.cpp)")
    ap.add_argument("--rccl-direct", action="store_true", help="(default since round 3; kept for old command lines)")
    ap.add_argument("--saturated-detector", action="store_true", help="keep the plain random fill of the detector: every class score saturates to 1.0, the ties defeat the detections_per_img cap and the mask head sees 200-300 detections per frame")
    ap.add_argument("--oversubscribe", action="store_true", help="N > 1 on a ONE-GPU box: every rank uses GPU 0, the process group is gloo and the sharded BA's all-reduce goes through host memory "
                                                                 "(host.host_allreduce_hook).  Numbers are meaningless; the point is that the launcher, the N-rank code path and the N > 1 JSON line "
                                                                 "have executed end to end before an 8-GPU node sees them (tests/test_e2e_gpu.py)")
    ap.add_argument("--gba-cams", type=int, default=500)
    ap.add_argument("--gba-points", type=int, default=100000)
    ap.add_argument("--full", action="store_true", help="after the headline, run every side measurement as well: the chain without the detector and with the networks' maps, the "
                                                        "networks alone with their FLOP/s, the rooflines and kernel figures, the optimisers / BA / matcher extras and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the chain handed its caller for the last timed frame as DIR/<name>.npy (rank 0): the tracker's "
                                                          "Tcw and point / object counts, the networks' flow / depth / label image and the detector's labels and counts; float32, at most 64 MB")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: spawn the N ranks the driver's launcher would (one process per GPU, RCCL over xGMI) and pass their line through
        import socket, subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    if args.gpus > 1 and world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the hot path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    if args.oversubscribe:
        local_rank = 0                                      # all ranks on the one GPU of the box
    torch.cuda.set_device(local_rank)
    os.environ["VIDO_DEVICE"] = str(local_rank)            # the System's tracker context (facade) follows the rank's GPU
    dist = None
    if world > 1:
        import torch.distributed as dist
        if args.oversubscribe:
            dist.init_process_group("gloo")                # (RCCL refuses two ranks on one device)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if dist is not None:
        dist.barrier()
    import ctypes as C
    import vido_slam_amd as V
    from vido_slam_amd import synth, pipeline
    from vido_slam_amd.system import System

    W, H = args.width, args.height

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # =============================================================================================================================
    # HEADLINE: the chained, pipelined end-to-end frame rate
    n_total = args.prologue + args.warmup + args.steps
    scene = synth.convoy_scene(n_total + 1, w=W, h=H, seed=5 + 100 * rank)

    def render(k):
        g, d, f, m = scene.frame(k)
        return synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)
    # Scene3D.frame(k) only reads the scene and numpy releases the GIL inside its array operations: a pool of host threads renders the same frames (~0.25 s each on
    # one core) several times faster than one loop.  At most 16 threads, shared by the ranks of one node.
    from concurrent.futures import ThreadPoolExecutor
    n_threads = max(1, min(16, len(os.sched_getaffinity(0))) // int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    with ThreadPoolExecutor(max_workers=n_threads) as pool:
        frames = list(pool.map(render, range(n_total)))
    tmp = tempfile.mkdtemp(prefix="vido_bench_")
    cfg_path = os.path.join(tmp, "settings.yaml")
    write_settings(cfg_path, scene.K, W, H)
    net_ctx = V.Context(device=local_rank, width=W, height=H, max_batch=1)             # owns the HIP ops of the network nodes (correlation, ROI-Align, NMS ...)
    t_setup = time.perf_counter()
    nodes = pipeline.NetNodes(net_ctx, H, W, optimize=not args.no_fold, graphs=not args.no_graphs, streams=(True if args.streams else (False if args.net_streams in ("none", "") else args.net_streams)), miopen_find=args.miopen_find, calibrate_scores=not args.saturated_detector,
                              static_detector=not args.saturated_detector)      # saturated scores tie at the detections_per_img cut on every frame: the fixed-slot head would fall back every time
    t_setup = time.perf_counter() - t_setup
    slam = System(); slam.Init(cfg_path, System.RGBD)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed=args.feed, handover=args.handover)

    def run(lo, hi):
        for k in range(lo, hi):
            bgr, d, f, m = frames[k]
            e2e.push(bgr, (d, f, m))
            if args.no_pipeline:
                e2e.finish()
        e2e.finish()

    run(0, args.prologue)                                    # fills the local-BA window (untimed set-up)
    run(args.prologue, args.prologue + args.warmup)          # W warm-up steps
    n0 = len(e2e.stats)
    sync_all()
    t0 = time.perf_counter()
    run(args.prologue + args.warmup, n_total)
    sync_all()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device="cpu" if args.oversubscribe else "cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        # the last timed frame, read after the clock: the tracker's pose and counts, and the networks' maps as parked in the frame's hand-over slot (the next push() reuses
        # the slot; with feed=given the tracker is handed the renderer's maps, the networks' are computed and parked all the same)
        slot = (e2e.k - 1) % e2e.RING
        db, hb = e2e.dev[slot], e2e.host[slot]
        outs = {"flow": db["flow"].cpu().numpy(), "depth": db["depth"].cpu().numpy(), "mask": db["mask"].cpu().numpy(), "det_labels": e2e._alive[3].cpu().numpy()}
        if nodes.last_counts is not None:
            outs["det_counts"] = hb["counts"].numpy().copy()                     # (labels kept, detections)
        if e2e.poses[-1] is not None:
            outs["pose_Tcw"] = e2e.poses[-1]
            outs["track_counts"] = np.array([e2e.stats[-1][k] for k in ("n_keypoints", "n_static", "n_static_inliers", "n_objects", "n_object_points", "ba_window")])
        dump_outputs(args.dump_outputs, outs)
    fps = args.steps * world / dt
    st = e2e.stats[n0:]
    mean = lambda key: float(np.mean([s.get(key, 0.0) for s in st])) if st else 0.0
    # pose accuracy of the timed frames against the renderer's ground truth: the chain did real work
    t_err = []
    for i, T in enumerate(e2e.poses):
        if T is None:                                        # VIDO_E2E_SKIP_TRACK=1 (diagnosis: the chain without the tracker)
            t_err.append(0.0); continue
        E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(i))
        t_err.append(float(np.linalg.norm(E[:3, 3])))
    stage = {"track_total_ms": mean("ms_total"), "update_mask_ms": mean("ms_update_mask"), "frame_orb_lists_ms": mean("ms_frame"), "cam_pose_ms": mean("ms_cam_pose"),
             "obj_tracking_ms": mean("ms_obj_tracking"), "obj_motion_ms": mean("ms_obj_motion"), "renew_ms": mean("ms_renew"), "local_ba_ms": mean("ms_local_ba"),
             "net_enqueue_host_ms": float(np.mean(e2e.t_net[n0:])), "tracker_wait_for_nets_ms": float(np.mean(e2e.t_wait[n0:])), "tracker_thread_ms": float(np.mean(e2e.t_track[n0:])),
             "tracker_wait_inputs_ms": mean("ms_wait_inputs"), "orb_ms": mean("ms_orb"), "lists_ms": mean("ms_lists")}
    stage["tracker_work_ms"] = stage["tracker_thread_ms"] - stage["tracker_wait_inputs_ms"]      # the thread's time minus its wait for the frame's networks (an event the tracker's stream is ordered behind)
    counts = {"keypoints": mean("n_keypoints"), "static_points": mean("n_static"), "static_inliers": mean("n_static_inliers"), "dynamic_objects": mean("n_objects"),
              "object_points": mean("n_object_points"), "ba_window": mean("ba_window")}
    counts["detector_detections"] = float(np.mean(e2e.n_det[n0:])) if len(e2e.n_det) > n0 else 0.0      # what the mask head ran on (reference cap: detections_per_img = 100)
    e2e.close()

    # ---- the chain exactly as BASELINE's metric text words it ("flow+depth+track+local-BA"): the same pipeline with the detector left out (the tracker is handed the
    # renderer's mask either way, feed=given).  Reported next to the headline, which keeps the harder chain (the tracker needs a mask: configs[2] names Mask R-CNN).
    e2e_nodet = None
    if args.full and world == 1 and not args.no_extra and not args.no_pipeline and args.feed == "given":
        try:
            slam.close()                                         # (one System per process at a time: the facade keeps its context in statics, as the reference's Frame does)
            slam2 = System(); slam2.Init(cfg_path, System.RGBD)
            nodes.skip_detector = True
            e2b = pipeline.EndToEnd(nodes, slam2, n_image=10 ** 6, feed=args.feed, handover=args.handover)
            def run2(lo, hi):
                for k in range(lo, hi):
                    bgr, d, f, m = frames[k]
                    e2b.push(bgr, (d, f, m))
                e2b.finish()
            nsteps2 = min(args.steps, 60)
            run2(0, args.prologue); run2(args.prologue, args.prologue + args.warmup)
            torch.cuda.synchronize(); t0b = time.perf_counter()
            run2(args.prologue + args.warmup, args.prologue + args.warmup + nsteps2)
            torch.cuda.synchronize(); dtb = time.perf_counter() - t0b
            e2b.close(); nodes.skip_detector = False
            st2 = e2b.stats[-nsteps2:]; m2 = lambda key: round(float(np.mean([x.get(key, 0.0) for x in st2])), 3) if st2 else 0.0
            e2e_nodet = {"frames_per_s": round(nsteps2 / dtb, 2), "ms_per_step": round(dtb / nsteps2 * 1e3, 3), "steps": nsteps2,
                         "stage_ms": {"track_total_ms": m2("ms_total"), "frame_orb_lists_ms": m2("ms_frame"), "orb_ms": m2("ms_orb"), "update_mask_ms": m2("ms_update_mask"), "cam_pose_ms": m2("ms_cam_pose"),
                                      "obj_motion_ms": m2("ms_obj_motion"), "renew_ms": m2("ms_renew"), "local_ba_ms": m2("ms_local_ba"), "tracker_wait_inputs_ms": m2("ms_wait_inputs"),
                                      "tracker_thread_ms": round(float(np.mean(e2b.t_track[-nsteps2:])), 3), "net_enqueue_host_ms": round(float(np.mean(e2b.t_net[-nsteps2:])), 3)},
                         "chain": "LiteFlowNet + MonoDepth2 -> device hand-over -> System::TrackRGBD -> PartialBatchOptimization (no Mask R-CNN launch; same frames, same pipelining)"}
            slam = slam2
        except Exception as e:
            e2e_nodet = {"error": "%s: %s" % (type(e).__name__, e)}; nodes.skip_detector = False
            slam = None

    # ---- the same chain with the tracker consuming the NETWORKS' maps (--feed nets): with random-init weights they carry no geometry, so the tracker's point counts differ
    # (reported); what the number shows is that the data dependency costs nothing beyond the completion event the headline already waits for
    e2e_feed_nets = None
    if args.full and world == 1 and not args.no_extra and not args.no_pipeline and args.feed == "given" and slam is not None:
        try:
            slam.close()
            slam3 = System(); slam3.Init(cfg_path, System.RGBD)
            e2c = pipeline.EndToEnd(nodes, slam3, n_image=10 ** 6, feed="nets", handover=args.handover)
            def run3(lo, hi):
                for k in range(lo, hi):
                    bgr, d, f, m = frames[k]
                    e2c.push(bgr, (d, f, m))
                e2c.finish()
            nsteps3 = min(args.steps, 40)
            run3(0, args.prologue); run3(args.prologue, args.prologue + args.warmup)
            torch.cuda.synchronize(); t0c = time.perf_counter()
            run3(args.prologue + args.warmup, args.prologue + args.warmup + nsteps3)
            torch.cuda.synchronize(); dtc = time.perf_counter() - t0c
            e2c.close()
            st3 = e2c.stats[-nsteps3:]; m3 = lambda key: round(float(np.mean([x.get(key, 0.0) for x in st3])), 3) if st3 else 0.0
            e2e_feed_nets = {"frames_per_s": round(nsteps3 / dtc, 2), "ms_per_step": round(dtc / nsteps3 * 1e3, 3), "steps": nsteps3,
                             "per_frame_counts": {"keypoints": m3("n_keypoints"), "static_points": m3("n_static"), "static_inliers": m3("n_static_inliers"), "dynamic_objects": m3("n_objects"), "object_points": m3("n_object_points")},
                             "stage_ms": {"track_total_ms": m3("ms_total"), "local_ba_ms": m3("ms_local_ba"), "tracker_thread_ms": round(float(np.mean(e2c.t_track[-nsteps3:])), 3)},
                             "chain": "the headline's chain with System::TrackRGBDDevice handed the networks' own flow / depth / mask (device ring slots; random-init weights: no geometry in them)"}
            slam = slam3
        except Exception as e:
            e2e_feed_nets = {"error": "%s: %s" % (type(e).__name__, e)}
            slam = None

    # ---- the three networks alone (sequential, one stream each in turn): ms per forward and fp32 FLOP/s against the 157.3 TFLOP/s peak
    roofline_nets = {}
    if args.full:
        try:
            ex = torch.as_tensor(frames[-1][0], device="cuda"); ex0 = torch.as_tensor(frames[-2][0], device="cuda")
            def timed(fn, reps=5):
                fn(); torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record(); torch.cuda.synchronize()
                return a.elapsed_time(b) / reps
            from torch.utils.flop_counter import FlopCounterMode
            def flops(fn):
                hops = [o for o in (nodes.ops, getattr(nodes, "ops_flow", None)) if o is not None]
                for o in hops:
                    o.gconv_flops = 0.0                                       # convolutions run by csrc/gconv.hip / conv1x1.hip / wino.hip are not torch ops: counted by the wrappers
                with FlopCounterMode(display=False) as fc:                    # (as the direct convolutions they replace)
                    fn()
                return float(fc.get_total_flops()) + sum(float(getattr(o, "gconv_flops", 0.0)) for o in hops)
            legs = {"liteflownet": (lambda: (nodes.g_flow or nodes._flow_fn)(ex0, ex), lambda: nodes._flow_fn(ex0, ex)),
                    "monodepth2": (lambda: (nodes.g_depth or nodes._depth_fn)(ex), lambda: nodes._depth_fn(ex)),
                    "maskrcnn_x101_fpn": ((lambda: nodes.g_det(ex)) if nodes.g_det is not None else
                                          (lambda: V.nets.analyse_image(nodes.mask_net, ex, feed=nodes.mask_feed, confidence=nodes.confidence, trunk=nodes.g_trunk)),
                                          lambda: V.nets.analyse_image(nodes.mask_net, ex, feed=nodes.mask_feed, confidence=nodes.confidence))}
            for name, (fast, eager) in legs.items():
                ms = timed(fast); fl = flops(eager)
                stage[name + "_ms"] = round(ms, 3)
                roofline_nets[name] = {"bound": "mfma", "achieved": round(fl / (ms * 1e-3) / 1e12, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                       "frac": round(fl / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4), "gflop_per_frame": round(fl / 1e9, 1), "ms": round(ms, 3), "dtype": "fp32",
                                       "note": "fp32-equivalent FLOPs of the node / its graph's replay time against the fp32 matrix instruction's peak; layers that compute their fp32 results on the 16-bit matrix instructions (config.net_arith) can take the fraction past 1"}
            stage["nets_sum_ms"] = round(sum(stage[k + "_ms"] for k in legs), 3)
            # the largest hand-written network kernel, alone: csrc/wino.hip on the detector's FPN / RPN convolution at P2 (256 -> 256 on 200 x 272), bias + ReLU included.
            # `achieved` counts the multiply-adds the kernel ISSUES to the matrix pipe (Winograd domain: 16 per 2x2 output tile and channel pair instead of 36); `direct_equivalent`
            # is the same launch priced as the direct convolution it replaces (what roofline_nets and the library's kernels are priced as).
            if hasattr(nodes.ops, "wino3x3_bias_act"):
                from vido_slam_amd.nets.ops import pack_wino3x3
                wx = torch.randn(1, 256, 200, 272, device="cuda"); ww = torch.randn(256, 256, 3, 3) / 48.0; wb = torch.randn(256, device="cuda"); wu = pack_wino3x3(ww).cuda()
                wms = timed(lambda: nodes.ops.wino3x3_bias_act(wx, wu, wb, 256, 0.0), reps=20)
                direct = 2.0 * 9 * 256 * 256 * 200 * 272
                roofline_nets["wino3x3_fpn_p2"] = {"kernel": "k_wino3x3<2,2,8>", "bound": "mfma", "achieved": round(direct * 16.0 / 36.0 / (wms * 1e-3) / 1e12, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                                   "frac": round(direct * 16.0 / 36.0 / (wms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4), "direct_equivalent_tflops": round(direct / (wms * 1e-3) / 1e12, 1),
                                                   "avg_launch_ms": round(wms, 4), "workgroups": 852, "dtype": "fp32"}
                del wx, ww, wb, wu
        except Exception as e:
            roofline_nets["error"] = "%s: %s" % (type(e).__name__, e)

    out = {
        "metric": "frames/sec end-to-end (flow+depth+track+local-BA) at 640x480; BA iters/sec",
        "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[1]+[2]+[3] chained: per %dx%d frame LiteFlowNet + MonoDepth2 (640x192 feed) + Mask R-CNN X-101-32x8d-FPN (800x1088 feed), fp32 batch 1, random-init weights "
                               "-> %s hand-over -> System::TrackRGBD (cvtColor, ORB 2000 features, lists, mask propagation, P3P-RANSAC, Flow2Cam, scene flow, object tracking, "
                               "per-object Flow2, re-seeding) -> PartialBatchOptimization over a full 20-frame window; networks of frame k+1 overlap tracking of frame k" % (W, H, "device-resident" if args.handover == "device" else "pinned-host"),
                   "frames_per_step": 1, "pipelined": not args.no_pipeline, "tracker_feed": args.feed,
                   "net_arith": ("fp32 instructions throughout" if os.environ.get("VIDO_CONV1X1_ARITH") == "f32" or os.environ.get("VIDO_NO_CONV1X1") or (os.environ.get("VIDO_CONV1X1_TN") and not os.environ.get("VIDO_CONV1X1_ARITH"))
                                 else "bf16x3-split, 6 products, fp32 accumulate (1x1 convolutions of the detector: csrc/conv1x1.hip::k_conv1x1_b3<NP 3>; every other layer on the fp32 matrix / vector instructions)" if os.environ.get("VIDO_CONV1X1_ARITH") in ("bf16x3", "bf16")
                                 else "f16x2-split (per-channel power-of-two weight scales, low planes x 2^11), 3 products, fp32 accumulate (1x1 convolutions of the detector: csrc/conv1x1.hip::k_conv1x1_b3<NP 2>; dense 3x3 layers on launches of >= 128 workgroups: csrc/conv3x3h.hip, the same arithmetic; every other layer on the fp32 matrix / vector instructions)"),
                   "handover": args.handover,
                   "tracker_feed_note": "networks run at full cost and their outputs are parked in the hand-over ring; with random-init weights those maps carry no geometry, so the tracker is "
                                        "handed the renderer's exact flow/depth/mask of the same frame (feed=given; uploaded next to the BGR frame) once the networks of that frame have completed",
                   "prologue_frames": args.prologue, "parallelism": "replicas x%d (per-frame path does not shard)" % world,
                   "net_optimisations": {"frozen_bn_folded_pairs": nodes.folded, "hip_graphs": nodes.g_flow is not None, "graph_error": nodes.graph_error,
                                         "network_streams": (1 if nodes.streams is None else len({id(x) for x in nodes.streams if x is not None}) + (1 if any(x is None for x in nodes.streams) else 0)), "detector_one_graph": nodes.g_det is not None, "detector_overflow_frames": nodes.det_overflows, "detector_score_calibration": round(nodes.score_scale, 6), "miopen_find": bool(args.miopen_find)},
                   "inputs": "BGR u8 frames in pinned host memory, one upload per frame; " + (
                       ("the networks' flow f32x2 / depth f32 / mask i32 are parked in the device ring and handed to System::TrackRGBDDevice as device pointers (no map crosses PCIe)" if args.feed == "nets" else
                        "the networks' flow / depth / mask are parked in the device ring (no download); feed=given: the renderer's flow f32x2 / depth f32 / mask i32 of the frame (4.9 MB) are UPLOADED next "
                        "to the BGR frame and those device buffers are what System::TrackRGBDDevice is handed — the networks -> tracker dependency in the timed chain is the completion event, not the data")
                       if args.handover == "device" else "flow f32x2 / depth f32 / mask i32 copied to pinned host buffers and handed to TrackRGBD")},
        "stage_ms": {k: round(v, 3) for k, v in stage.items()},
        "per_frame_counts": {k: round(v, 1) for k, v in counts.items()},
        "pose_translation_error_m": {"mean": round(float(np.mean(t_err[1:])), 4), "max": round(float(np.max(t_err[1:])), 4), "path_length_m": round(0.25 * (len(t_err) - 1), 2)},
        "net_setup_s": round(t_setup, 1),
        "parity_pin": "nets pinned by reference fixtures (LiteFlowNet, MonoDepth2 decoder, Mask R-CNN stage by stage; NMS / box decode by the reference's own KATs; ROI-Align and the "
                      "ResNet-18 encoder by independent float64 implementations written from the reference text); ORB / tracker / RANSAC / BA UNPINNED: the reference's OpenCV + g2o "
                      "core cannot be built in this image (no OpenCV / Eigen / CXSparse) and has no tests or fixtures of its own",
        "targets": {"north_star_frames_per_s": 200, "fp32_flop_floor_ms_per_frame": round((888.7 + 200.5 + 16.0) / FP32_PEAK_TFLOPS, 2),
                    "note": "1.105 TFLOP of fp32 convolutions per frame / 157.3 TFLOP/s = 7.0 ms > the 5 ms a 200 frames/s chain has: unreachable on the fp32 matrix instruction alone; "
                            "the split-fp16 form of the 1x1 layers (round 6) is the first step under that floor"},
    }
    del e2e, slam
    if not args.full:                                        # a plain run ends with its headline
        if rank == 0:
            print(json.dumps(out))
        if dist is not None:
            dist.destroy_process_group()
        return
    out["roofline_nets"] = roofline_nets

    # =============================================================================================================================
    # roofline of the dominant hand-written front-end kernel, on configs[1] batched (64 frames in flight)
    B = args.batch
    extra = {}
    if e2e_nodet is not None:
        extra["e2e_without_detector"] = e2e_nodet
    if e2e_feed_nets is not None:
        extra["e2e_feed_nets"] = e2e_feed_nets
    try:
        ctx = V.Context(device=local_rank, width=W, height=H, max_batch=B)
        tp = V.track_params(dataset=0, depth_map_factor=1.0, th_depth_bg=40.0, th_depth_obj=25.0)
        ff = V.FrameFeatures(ctx, tp)
        n_distinct = min(B, 16)
        seq = synth.Sequence(n_frames=n_distinct, w=W, h=H, seed=1 + 100 * rank)
        fr = [seq.frame(k) for k in range(n_distinct)]
        sel = np.arange(B) % n_distinct
        gray_h = np.ascontiguousarray(np.stack([fr[i][0] for i in sel]))
        depth_h = np.ascontiguousarray(np.stack([fr[i][2] for i in sel]).astype(np.float32))
        flow_h = np.ascontiguousarray(np.stack([fr[i][3] for i in sel]))
        mask_h = np.ascontiguousarray(np.stack([fr[i][4] for i in sel]))
        gray_d = torch.from_numpy(gray_h).cuda(); depth_d = torch.from_numpy(depth_h).cuda()
        flow_d = torch.from_numpy(flow_h).cuda(); mask_d = torch.from_numpy(mask_h).cuda()
        bsteps, bwarm = 20, 3
        depth_pool = [depth_d.clone() for _ in range(bsteps + bwarm)]      # the pre-scale rewrites its input in place: a fresh raw batch per step, resident before timing
        torch.cuda.synchronize()
        dev_arg = (gray_d.data_ptr(), B, H, W, H * W, W)
        stage_b = {}
        for i in range(bwarm):
            ff.frontend_batch(0, dev_arg, depth_pool[i].data_ptr(), flow_d.data_ptr(), mask_d.data_ptr(), alias=True)
        torch.cuda.synchronize(); tb = time.perf_counter()
        for i in range(bsteps):
            o = ff.frontend_batch(0, dev_arg, depth_pool[bwarm + i].data_ptr(), flow_d.data_ptr(), mask_d.data_ptr(), alias=True)
            for k, v in ctx.orb_timing().items():
                stage_b[k] = stage_b.get(k, 0.0) + v / bsteps
        torch.cuda.synchronize(); tb = time.perf_counter() - tb
        p_px = 0
        for l in range(ctx.cfg.n_levels):
            a, b = C.c_int(), C.c_int()
            ctx.lib.vido_orb_level_size(ctx.h, l, C.byref(a), C.byref(b))
            p_px += a.value * b.value
        fast_bytes = p_px * B + 4.0 * stage_b.get("n_candidates", 0.0)     # every pyramid pixel read once (950 532 B per 640x480 frame) + 4 B per candidate
        fast_s = stage_b["fast_ms"] * 1e-3
        ach = fast_bytes / fast_s / 1e9 if fast_s > 0 else 0.0
        roofline = {"kernel": "FAST stage (score map + per-cell selection)", "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": None, "algorithmic_bytes_per_launch": int(fast_bytes), "avg_launch_ms": round(stage_b["fast_ms"], 4),
                    "workload": "configs[1] batched: %d frames of %dx%d in flight" % (B, W, H)}
        rel, pmc_path = newest_profile("pmc_traffic.json")
        if pmc_path and B == 64 and (W, H) == (640, 480):
            ks = json.load(open(pmc_path))["kernels"]
            tot = 0.0; names = []
            for name, k in ks.items():
                if name.startswith("k_fast"):
                    tot += (2.0 * k["FETCH_SIZE_KB_mean_per_launch"] + k["WRITE_SIZE_KB_mean_per_launch"]) * 1024; names.append(name)
            if names:
                roofline["traffic"] = int(tot)
                roofline["traffic_source"] = "%s %s (rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE, separate passes; FETCH x2 gfx950 correction)" % (rel, "+".join(names))
        # what actually bounds the kernel: the integer vector ALUs, not HBM (the counted traffic equals the algorithmic bytes) — the wave-instruction count of a launch is read
        # from the newest committed SQ-counter pass (tools/pmc_fast.sh -> profiles/rN/fast_sq_counters.txt), 4 cycles each on a 16-lane SIMD; reported next to the HBM fraction
        rel, sq_path = newest_profile("fast_sq_counters.txt")
        if sq_path and fast_s > 0 and B == 64 and (W, H) == (640, 480):
            sq = read_sq_counters(sq_path)
            if sq.get("SQ_INSTS_VALU"):
                nv = sq["SQ_INSTS_VALU"]
                # cycles per wave-instruction per SIMD of the kernel's instruction class, MEASURED (tools/ubench/valu_int_issue.hip -> profiles/rN/valu_int_issue.txt): the
                # packed 16-bit / three-operand integer instructions issue at 3.24 cycles with 4 waves per SIMD and 2.62 with 8 — neither the 4 the round-5 line assumed nor
                # the 2 of the guide's v_fma_f32 row; k_fast_strips runs 5 waves per SIMD: interpolated
                cpi, cpi_src = 4.0, "assumed (no profiles/rN/valu_int_issue.txt)"
                urel, upath = newest_profile("valu_int_issue.txt")
                if upath:
                    for line in open(upath):
                        if line.startswith("v_pk_min_u16"):
                            cells = [float(c.split()[0]) for c in line.split("/")[1:]]      # per-SIMD figures at 1, 2, 4, 8 waves per SIMD
                            if len(cells) == 4:
                                cpi = round(cells[2] + (cells[3] - cells[2]) * 0.25, 3); cpi_src = "%s: v_pk_min_u16 at 4 / 8 waves per SIMD = %.2f / %.2f cycles, interpolated to the kernel's 5" % (urel, cells[2], cells[3])
                roofline["limiter"] = {"bound": "integer VALU issue", "valu_wave_instructions_per_launch": nv, "cycles_per_instruction": cpi, "cycles_per_instruction_source": cpi_src,
                                       "simds": 1024, "clock_ghz": 2.4, "frac_of_valu_issue_peak": round(nv * cpi / (1024 * 2.4e9 * fast_s), 3),
                                       "note": "clock_ghz is the nominal 2.4; the same micro-benchmark sustains ~1.7 GHz with every SIMD issuing (DVFS), so the kernel is closer to its issue bound than this fraction says",
                                       "source": "%s (rocprofv3 --pmc SQ_INSTS_VALU, per k_fast_strips launch)" % rel}
        out["roofline"] = roofline
        extra["configs1_frontend_batched"] = {"frames_per_s": round(B * bsteps / tb, 1), "ms_per_%d_frames" % B: round(tb / bsteps * 1e3, 4),
                                              "stage_ms": {k: round(v, 4) for k, v in stage_b.items() if k != "n_candidates"},
                                              "keypoints_per_frame": float(o["n_kp"].mean()), "note": "round-1 headline workload: ORB + depth pre-scale + frame lists, 64 frames in flight"}
    except Exception as e:
        import traceback
        out["roofline_error"] = "%s: %s" % (type(e).__name__, e); traceback.print_exc(file=sys.stderr)
        ctx = V.Context(device=local_rank, width=W, height=H, max_batch=1)

    # the side measurements include host-side C++ set-up that runs on the library's own worker threads: torch's OpenMP pool, still spinning after the pipeline's CPU-side tensor
    # ops, took their cores away (global BA set-up 4 ms in a fresh process, 12-22 ms behind a torch CPU op; profiles/r4/global_ba_setup_variance.txt)
    torch_threads = torch.get_num_threads(); torch.set_num_threads(1)
    if not args.no_extra:
      try:
          P = V.problems
          opt = V.Optimizer(ctx)
          s = P.synth_pose_scene(3000, seed=2)
          probs = {"PoseOptimizationFlow2Cam_N3000": P.pose_problem_flow2cam(s["uv_last"], s["flow"], s["depth"], s["Twl"], s["K"], s["T_init"]),
                   "PoseOptimizationNew_N3000": P.pose_problem_new(s["Xw"], s["uv_cur"], s["K"], s["T_init"])}
          for name, pr in probs.items():
              opt.pose_optimize(pr)
              t1 = time.perf_counter(); reps = 5
              for _ in range(reps):
                  r = opt.pose_optimize(pr)
              d = (time.perf_counter() - t1) / reps
              extra[name] = {"ms_per_call": round(d * 1e3, 3), "lm_iterations": r["lm_iterations"], "lm_iters_per_s": round(r["lm_iterations"] / d, 1)}
          # k_pose_opt, the largest hand-written kernel of the tracker's trace, against what bounds it.  SURVEY section 8d prices an LM iteration at ~56 B per residual
          # (168 KB at N = 3000): 0.02 us of HBM time — the kernel is a chain of dependent passes and exchanges, so what it is measured against is
          # the latency floor of that chain: 2 cluster exchanges (~3 us each) + 2 passes of one residual per thread (~2.5 us) per iteration.
          f2c = extra["PoseOptimizationFlow2Cam_N3000"]
          us_it = f2c["ms_per_call"] * 1e3 / max(f2c["lm_iterations"], 1)
          out["roofline_pose_opt"] = {"kernel": "k_pose_opt", "workload": "PoseOptimizationFlow2Cam, N = 3000 (6 workgroups of 512 threads, one residual per thread)", "bound": "latency",
                                      "lm_iterations_per_s": f2c["lm_iters_per_s"], "us_per_lm_iteration_whole_call": round(us_it, 2), "hbm_floor_us_per_iteration": round(168e3 / (HBM_PEAK_GBS * 1e9) * 1e6, 4),
                                      "note": "a chain of dependent passes and cluster exchanges per LM iteration (DESIGN.md): measured against HBM time it is 1e-3 of the roofline by construction; no latency floor is claimed here"}
          objs = []
          for k in range(5):
              so = P.synth_pose_scene(800, seed=30 + k)
              objs.append(P.pose_problem_flow2(so["uv_last"], so["flow"], so["depth"], so["Twl"], so["K"], so["T_init"]))
          opt.pose_optimize_batch(objs)
          t1 = time.perf_counter()
          for _ in range(5):
              rs = opt.pose_optimize_batch(objs)
          d = (time.perf_counter() - t1) / 5
          extra["PoseOptimizationFlow2_5objects_x800"] = {"ms_per_frame": round(d * 1e3, 3), "lm_iterations": [r["lm_iterations"] for r in rs]}
          for na, nb in ((2000, 2000), (128000, 2000)):
              da = torch.randint(0, 256, (na, 32), dtype=torch.uint8, device="cuda"); db = torch.randint(0, 256, (nb, 32), dtype=torch.uint8, device="cuda")
              mi = torch.empty(na, dtype=torch.int32, device="cuda"); md = torch.empty(na, dtype=torch.int32, device="cuda")
              torch.cuda.synchronize()
              runh = lambda: (ctx.hamming_match_device(da.data_ptr(), na, db.data_ptr(), nb, mi.data_ptr(), md.data_ptr()), ctx.synchronize())
              runh(); t1 = time.perf_counter(); reps = 10
              for _ in range(reps):
                  runh()
              d = (time.perf_counter() - t1) / reps
              extra["hamming_%dx%d" % (na, nb)] = {"ms_per_call": round(d * 1e3, 4), "pairs_per_s": round(na * nb / d, 0), "descriptor_GB_per_s": round(32.0 * (na + nb) / d / 1e9, 2)}
          # the detector's grouped 3x3 convolution on the matrix cores (csrc/gconv.hip): the hand-written kernel with the most GPU time per frame in the headline
          # (22 launches of the 32-channels-per-group shape); fp32 FLOPs of the convolution / HIP-event time on the stream it is launched on
          try:
              from vido_slam_amd.nets.ops import HipOps, pack_gconv3x3
              gops = HipOps(ctx); rg = {}
              for cpg, gh, gw, per_frame in ((32, 50, 68, 22), (16, 100, 136, 3), (8, 200, 272, 3), (64, 25, 34, 2)):
                  gx = torch.randn(1, 32 * cpg, gh, gw, device="cuda"); gwt = torch.randn(32 * cpg, cpg, 3, 3, device="cuda") * 0.05; gb = torch.randn(32 * cpg, device="cuda")
                  gp = pack_gconv3x3(gwt, 32)
                  for _ in range(5):
                      gops.gconv3x3_bias_act(gx, gp, gb, 32, 0.0, in_bias=gb)
                  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True); reps = 100
                  e0.record()
                  for _ in range(reps):
                      gops.gconv3x3_bias_act(gx, gp, gb, 32, 0.0, in_bias=gb)
                  e1.record(); torch.cuda.synchronize()
                  us = e0.elapsed_time(e1) * 1e3 / reps; fl = 2.0 * 32 * cpg * cpg * 9 * gh * gw
                  rg["%d_channels_per_group_%dx%d" % (cpg, gh, gw)] = {"us_per_launch": round(us, 2), "achieved": round(fl / us / 1e6, 2), "launches_per_frame": per_frame}
              main = rg["32_channels_per_group_50x68"]
              out["roofline_gconv"] = {"kernel": "k_gconv3x3_m32 (grouped 3x3 convolution + both folded batch norms + ReLUs, fp32 matrix cores)", "bound": "mfma", "achieved": main["achieved"],
                                       "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(main["achieved"] / FP32_PEAK_TFLOPS, 4), "traffic": None,
                                       "flops_per_launch": 2.0 * 1024 * 32 * 9 * 50 * 68, "shapes": rg,
                                       "note": "algorithmic FLOPs of the convolution (pad positions and the zero half of the 8-channel form not counted) / HIP-event time of 100 back-to-back launches"}
          except Exception as e:
              out["roofline_gconv_error"] = "%s: %s" % (type(e).__name__, e)
          # the detector's 1x1 convolutions in the split form (csrc/conv1x1.hip::k_conv1x1_b3): fp32-equivalent FLOPs / HIP-event time; the peak of this form is the
          # 16-bit matrix peak / the products per fp32 multiply-add (3 for the fp16 form, 6 for the bf16 form)
          try:
              from vido_slam_amd.nets.ops import HipOps, pack_conv1x1
              cops1 = HipOps(ctx); rc = {}
              for cin, cout, ch, cw, per_frame, nm in ((1024, 1024, 50, 68, 46, "layer3"), (512, 512, 100, 136, 8, "layer2"), (256, 256, 200, 272, 6, "layer1"), (2048, 2048, 25, 34, 5, "layer4")):
                  lay = cops1.conv1x1_layout(cin, cout, ch * cw)
                  cx = torch.randn(1, cin, ch, cw, device="cuda"); cwt = torch.randn(cout, cin, 1, 1) / cin ** 0.5; cb = torch.randn(cout, device="cuda"); cr = torch.randn(1, cout, ch, cw, device="cuda")
                  cp = pack_conv1x1(cwt, lay).cuda()
                  for _ in range(5):
                      cops1.conv1x1_bias_act(cx, cp, cb, cr, 0.0)
                  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True); reps = 100
                  e0.record()
                  for _ in range(reps):
                      cops1.conv1x1_bias_act(cx, cp, cb, cr, 0.0)
                  e1.record(); torch.cuda.synchronize()
                  us = e0.elapsed_time(e1) * 1e3 / reps; fl = 2.0 * cin * cout * ch * cw
                  rc["%s_%d_to_%d_at_%dx%d" % (nm, cin, cout, ch, cw)] = {"us_per_launch": round(us, 2), "fp32_equivalent_tflops": round(fl / us / 1e6, 1), "layout": lay, "launches_per_frame_about": per_frame}
              mainc = rc["layer3_1024_to_1024_at_50x68"]; split = mainc["layout"] >= 2; nprod = {2: 6, 3: 3}.get(mainc["layout"], 1); npl = {2: 3, 3: 2}.get(mainc["layout"], 2)
              pk = 2500.0 / nprod if split else FP32_PEAK_TFLOPS
              # operand bytes a launch moves L2 -> LDS: per 128 x 128 tile and input channel 128 weights x 2 bytes x planes + 128 activations x 4 bytes
              tiles3 = (1024 // 128) * ((50 * 68 + 127) // 128); stream = tiles3 * 1024 * (128 * 2 * npl + 128 * 4)
              out["roofline_conv1x1"] = {"kernel": ("k_conv1x1_b3<NP 2> (1x1 convolution + bias + residual + ReLU; two fp16 planes per fp32 operand, three products on v_mfma_f32_32x32x16_f16, fp32 accumulate)" if nprod == 3 else
                                                    "k_conv1x1_b3<NP 3> (1x1 convolution + bias + residual + ReLU; three bf16 planes per fp32 operand, six products on v_mfma_f32_32x32x16_bf16, fp32 accumulate)") if split else "k_conv1x1 (fp32 matrix instruction)",
                                         "bound": "mfma", "achieved": mainc["fp32_equivalent_tflops"], "peak": round(pk, 1), "unit": "TFLOP/s", "frac": round(mainc["fp32_equivalent_tflops"] / pk, 4),
                                         "traffic": _split_pmc("k_conv1x1_b3_1024_to_1024_at_50x68") if nprod == 3 else None, "traffic_source": "profiles/rN/split_kernels_pmc.json (rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE, separate passes; FETCH x2)",
                                         "tflops_16bit_issued": round(mainc["fp32_equivalent_tflops"] * nprod, 1) if split else None, "shapes": rc,
                                         "operand_stream": {"bytes_l2_to_lds_per_launch": stream, "tb_per_s": round(stream / mainc["us_per_launch"] / 1e6, 2),
                                                            "note": "every 128 x 128 tile streams its own weight planes and activations through LDS: what the launch's time follows (DESIGN.md 4d), not the matrix pipe"} if split else None,
                                         "note": "fp32-equivalent FLOPs (2 cin cout H W) / HIP-event time of 100 back-to-back launches with bias + residual + ReLU; peak = 2500 TFLOP/s dense 16-bit / products per multiply-add; "
                                                 "the fp32 matrix instruction's own peak is 157.3"}
          except Exception as e:
              out["roofline_conv1x1_error"] = "%s: %s" % (type(e).__name__, e)
          # the dense 3x3 layers: the direct split-fp16 kernel (csrc/conv3x3h.hip) and, beside it, the fp32 Winograd kernel it replaced on these launches
          try:
              from vido_slam_amd.nets.ops import HipOps, pack_conv3x3_h, pack_wino3x3
              cops3 = HipOps(ctx); r3 = {}
              for n3, cin, cout, ch, cw, nm in ((1, 256, 256, 200, 272, "fpn_rpn_p2"), (100, 256, 256, 14, 14, "mask_head"), (1, 256, 256, 100, 136, "fpn_rpn_p3"), (1, 128, 64, 120, 160, "liteflownet_128_to_64_level2")):
                  cx = torch.randn(n3, cin, ch, cw, device="cuda"); cwt = torch.randn(cout, cin, 3, 3) / (3 * cin ** 0.5); cb = torch.randn(cout, device="cuda")
                  wp3 = pack_conv3x3_h(cwt).cuda(); form = cops3.wino3x3_form(n3, cin, cout, ch, cw); u3 = pack_wino3x3(cwt, form).cuda()
                  def _t(fn, reps=30):
                      for _ in range(3): fn()
                      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                      e0.record()
                      for _ in range(reps): fn()
                      e1.record(); torch.cuda.synchronize()
                      return e0.elapsed_time(e1) * 1e3 / reps
                  us_h = _t(lambda: cops3.conv3x3_h_bias_act(cx, wp3, cb, cout, 0.0)); us_w = _t(lambda: cops3.wino3x3_bias_act(cx, u3, cb, cout, 0.0, form))
                  fl = 2.0 * n3 * cin * cout * 9 * ch * cw
                  r3["%s_%dx%d_to_%d_at_%dx%d" % (nm, n3, cin, cout, ch, cw)] = {"us_per_launch": round(us_h, 1), "fp32_equivalent_tflops": round(fl / us_h / 1e6, 1), "winograd_fp32_us": round(us_w, 1),
                                                                            "workgroups": int(cops3.ctx.lib.vido_conv3x3_h_workgroups(n3, cout, ch, cw))}
              m3 = r3["fpn_rpn_p2_1x256_to_256_at_200x272"]
              out["roofline_conv3x3"] = {"kernel": "k_conv3x3_h (direct 3x3 convolution + bias + ReLU; two fp16 planes per fp32 operand, three products on v_mfma_f32_32x32x16_f16, fp32 accumulate)",
                                         "bound": "mfma", "achieved": m3["fp32_equivalent_tflops"], "peak": round(2500.0 / 3, 1), "unit": "TFLOP/s", "frac": round(m3["fp32_equivalent_tflops"] / (2500.0 / 3), 4),
                                         "traffic": _split_pmc("k_conv3x3_h_256_to_256_at_200x272"), "traffic_source": "profiles/rN/split_kernels_pmc.json (FETCH x2 + WRITE; the window gathers are an uncalibrated width: raw FETCH + WRITE = 110.8 MB)",
                                         "shapes": r3, "note": "direct-convolution FLOPs (2 x 9 cin cout N H W) / HIP-event time of 30 back-to-back launches; peak = 2500 TFLOP/s dense fp16 / 3 products"}
          except Exception as e:
              out["roofline_conv3x3_error"] = "%s: %s" % (type(e).__name__, e)
          # configs[3] (static graph): 20 KF x 2k landmarks
          pr = P.synth_ba_problem(n_cam=20, n_pt=2000, kind="local", seed=7)
          V.ba_optimize(ctx, pr)
          t1 = time.perf_counter(); reps = 5
          for _ in range(reps):
              r = V.ba_optimize(ctx, pr)
          d = (time.perf_counter() - t1) / reps
          extra["local_ba_20kf_2k"] = {"ms_per_solve": round(d * 1e3, 3), "ms_lm_loop": round(r["ms_solve_loop"], 3), "ms_setup": round(r["ms_setup"], 3),
                                       "lm_iterations": r["iterations"], "lm_iters_per_s": round(r["iterations"] / (r["ms_solve_loop"] * 1e-3), 1),
                                       "n_obs": int(len(pr["obs_cam"])), "ms_linearize_kernel": round(r.get("ms_linearize_kernel", 0.0), 5)}

          def ba_roofline(r, n_obs, workload, pmc_file):
              if not r.get("ms_linearize_kernel", 0.0) > 0:
                  return None
              nb = 288.0 * n_obs
              ach = nb / (r["ms_linearize_kernel"] * 1e-3) / 1e9
              traffic = None
              for rnd in ("r3", "r2", "r1"):
                  try:
                      with open(os.path.join(ROOT, "profiles", rnd, pmc_file)) as fjs:
                          traffic = json.load(fjs)["kernels"]["k_ba_linearize"]["traffic_bytes_fetch_x2"]
                      break
                  except Exception:
                      pass
              return {"kernel": "k_ba_linearize", "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
                      "traffic": traffic, "algorithmic_bytes_per_launch": int(nb), "avg_launch_ms": round(r["ms_linearize_kernel"], 5), "workload": workload}
          rb = ba_roofline(r, len(pr["obs_cam"]), "configs[3] static graph, 20 KF x 2k landmarks", "pmc_traffic_ba.json")
          if rb:
              out["roofline_ba"] = rb
          # configs[4]: global BA, landmarks sharded over the ranks, RCCL all-reduce of the reduced camera system
          gpr = P.synth_ba_problem(n_cam=args.gba_cams, n_pt=args.gba_points, kind="global", track_len=10, seed=11)
          gpr["max_iters"] = 5
          shards = V.landmark_shards(gpr["obs_pt"], gpr["n_pt"], world)
          rccl_direct = not args.torch_allreduce and not args.oversubscribe
          hook = (V.host_allreduce_hook() if args.oversubscribe else (V.rccl_direct_init(ctx, rank, world) if rccl_direct else V.torch_allreduce_hook())) if world > 1 else None
          sync_all()
          t1 = time.perf_counter()
          r = V.ba_optimize(ctx, gpr, rank=rank, world=world, shard=shards[rank] if world > 1 else None, allreduce=hook)
          sync_all()
          d_cold = time.perf_counter() - t1
          t1 = time.perf_counter()
          r = V.ba_optimize(ctx, gpr, rank=rank, world=world, shard=shards[rank] if world > 1 else None, allreduce=hook)
          sync_all()
          d = time.perf_counter() - t1
          extra["global_ba"] = {"n_cam": args.gba_cams, "n_landmarks": int(gpr["n_pt"]), "n_obs": int(len(gpr["obs_cam"])), "n_gpus": world,
                                "lm_iterations": r["iterations"], "lm_trials": r["lm_trials"], "ms_lm_loop": round(r["ms_solve_loop"], 2),
                                "ms_setup": round(r["ms_setup"], 2), "lm_iters_per_s": round(r["iterations"] / (r["ms_solve_loop"] * 1e-3), 2),
                                "chi2": [round(r["chi2_initial"], 3), round(r["chi2_final"], 3)], "wall_ms": round(d * 1e3, 1), "wall_ms_first_call": round(d_cold * 1e3, 1),
                                "collective": ("gloo all-reduce through host memory (--oversubscribe: all ranks on one GPU)" if args.oversubscribe else "RCCL all-reduce (sum) of the reduced camera system per LM trial, " + ("issued by the library on its stream" if rccl_direct else "through the torch.distributed hook")) if world > 1 else "none",
                                "scaling_curve": "no 8-GPU scaling curve measured by the builder (single-GPU boxes); the driver's SCALE record is the measurement"}
          if r.get("ms_schur_kernel", 0.0) > 0:
              # the Schur kernel of the global path (k_ba_schur_mfma): per observation it reads the 27-double slot record the linearisation wrote (216 B), per landmark it writes
              # 3 doubles; the camera-pair blocks stay in LDS and leave once per chunk.  Counted traffic: read from the newest profiles/rN/pmc_traffic_ba_global.json.
              nb = 216.0 * len(gpr["obs_cam"]) + 24.0 * gpr["n_pt"]
              ach = nb / (r["ms_schur_kernel"] * 1e-3) / 1e9
              sch_traffic, sch_src = None, None
              rel, tp_ = newest_profile("pmc_traffic_ba_global.json")
              if tp_ and args.gba_cams == 500 and int(gpr["n_pt"]) == 100000:
                  for kn, kv in json.load(open(tp_))["kernels"].items():
                      if kn.startswith("k_ba_schur_mfma"):
                          sch_traffic = int((2.0 * kv["FETCH_SIZE_KB_mean_per_launch"] + kv["WRITE_SIZE_KB_mean_per_launch"]) * 1024); sch_src = "%s %s (FETCH x2 + WRITE)" % (rel, kn)
              out["roofline_ba_schur"] = {"kernel": "k_ba_schur_mfma", "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
                                          "traffic": sch_traffic, "traffic_source": sch_src, "algorithmic_bytes_per_launch": int(nb),
                                          "avg_launch_ms": round(r["ms_schur_kernel"], 5), "note": "FP64 matrix-core outer products per landmark chunk; bounded by the dependent chain per chunk, not by HBM"}
          if "ms_phases" in r:
              extra["global_ba"]["ms_phases_per_trial"] = r["ms_phases"]
          # the second half of BASELINE's metric ("BA iters/sec"), first-class: configs[4] sharded over the N ranks (landmark ranges, one all-reduce of the reduced camera
          # system per LM trial).  `wall` counts the whole call as a user sees it (host set-up + upload + LM loop + download), `lm_loop` the device loop only.
          out["global_ba_iters_per_s"] = {"wall": round(r["iterations"] / d, 2), "lm_loop": round(r["iterations"] / (r["ms_solve_loop"] * 1e-3), 2), "n_gpus": world,
                                          "workload": "configs[4]: %d KF x %d landmarks, %d observations, strong scaling over the ranks" % (args.gba_cams, int(gpr["n_pt"]), len(gpr["obs_cam"]))}
          if world == 1:
              rb = ba_roofline(r, len(gpr["obs_cam"]), "configs[4] size on one GPU: %d KF x %d landmarks, %d edges" % (args.gba_cams, int(gpr["n_pt"]), len(gpr["obs_cam"])), "pmc_traffic_ba_global.json")
              if rb:
                  out["roofline_ba_global"] = rb
          if rank == 0:
              dpr = P.synth_ba_problem(n_cam=200, n_pt=20000, kind="global", track_len=10, seed=13); dpr["max_iters"] = 5
              ddy = P.synth_ba_dynamic(dpr, n_obj=3, pts_per_obj=300, seed=14, max_len=8)
              t1 = time.perf_counter(); r = V.ba_optimize(ctx, dpr, dynamic=ddy); d = time.perf_counter() - t1
              extra["global_ba_dynamic"] = {"n_cam": 200, "n_H": int(ddy["n_H"]), "n_landmarks": int(dpr["n_pt"]), "n_obs": int(len(dpr["obs_cam"])), "n_dyn_points": int(ddy["n_dyn"]),
                                            "n_ternary": int(ddy["n_tern"]), "lm_iterations": r["iterations"], "ms_lm_loop": round(r["ms_solve_loop"], 2), "ms_setup": round(r["ms_setup"], 2),
                                            "lm_iters_per_s": round(r["iterations"] / (r["ms_solve_loop"] * 1e-3), 2), "chi2": [round(r["chi2_initial"], 3), round(r["chi2_final"], 3)],
                                            "wall_ms": round(d * 1e3, 1)}
          out["extra"] = extra
      except Exception as e:     # side measurements must never take the headline line down
        import traceback
        out["extra"] = extra
        out["extra_error"] = "%s: %s" % (type(e).__name__, e)
        traceback.print_exc(file=sys.stderr)
    else:
        out["extra"] = extra

    # =============================================================================================================================
    # CPU baseline of the same chain (rank 0, N = 1): networks on torch-CPU (the reference's Python modules are torch too) with the oracle's
    # correlation / ROI-Align / NMS / box decode, then the C oracle for ORB + lists + pose optimisers + local BA of one frame
    if rank == 0 and world == 1 and args.cpu_baseline > 0:
        try:
            from oracle import pyoracle as O
            torch.set_num_threads(torch_threads); nthreads = torch.get_num_threads()
            cops = O.OracleNetOps(O)
            corr = lambda a, b, s_: torch.from_numpy(O.correlation(a.numpy(), b.numpy(), s_))
            lfn = V.nets.fill_deterministic(V.nets.LiteFlowNet(corr), 1).eval()
            md = V.nets.fill_deterministic(V.nets.MonoDepth2(), 2).eval()
            mr = V.nets.fill_maskrcnn(V.nets.MaskRCNN(cops), 3).eval()
            P = V.problems
            op = O.orb_params(n_features=2000, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7)
            n_cam_pts = int(counts["static_inliers"]) or 1500
            sc = P.synth_pose_scene(n_cam_pts, seed=2)
            cam_pr = P.pose_problem_flow2cam(sc["uv_last"], sc["flow"], sc["depth"], sc["Twl"], sc["K"], sc["T_init"])
            obj_pr = []
            for k in range(5):
                so = P.synth_pose_scene(400, seed=30 + k)
                obj_pr.append(P.pose_problem_flow2(so["uv_last"], so["flow"], so["depth"], so["Twl"], so["K"], so["T_init"]))
            ba_pr = P.synth_ba_problem(n_cam=20, n_pt=2000, kind="local", seed=7)
            # (a) PRIMARY, BASELINE.md section 3: the SLAM stages — the reference's OpenCV + g2o CPU path as the oracle restates it — on ONE pinned core
            # (the reference library is single-threaded: g2o OpenMP OFF, 3rdparty/g2o/CMakeLists.txt:54), per-frame times over --cpu-baseline frames, median and p95
            aff0 = os.sched_getaffinity(0); pin = sorted(aff0)[len(aff0) // 2]
            os.sched_setaffinity(0, {pin})
            per_frame, parts = [], {}
            try:
                for i in range(args.cpu_baseline):
                    bgr, d, f, m = frames[-1 - (i % (len(frames) - 1))]
                    t0 = t1 = time.perf_counter()
                    g = O.bgr2gray(bgr)
                    kps, _, _ = O.orb_extract(op, g)
                    dpt = O.depth_prescale(d.copy(), 0, 1.0, 387.57, 1.0)
                    O.static_candidates(kps, dpt, f, m, 40.0); O.dense_object_samples(dpt, f, m, 25.0)
                    parts.setdefault("orb_lists_ms", []).append((time.perf_counter() - t1) * 1e3); t1 = time.perf_counter()
                    O.pose_optimize(cam_pr)
                    for pr_ in obj_pr:
                        O.pose_optimize(pr_)
                    parts.setdefault("pose_optimisers_ms", []).append((time.perf_counter() - t1) * 1e3); t1 = time.perf_counter()
                    O.ba_optimize(dict(ba_pr))
                    parts.setdefault("local_ba_ms", []).append((time.perf_counter() - t1) * 1e3)
                    per_frame.append((time.perf_counter() - t0) * 1e3)
            finally:
                os.sched_setaffinity(0, aff0)
            med = float(np.median(per_frame)); p95 = float(np.percentile(per_frame, 95))
            # (b) SEPARATE part: the three networks on torch-CPU fp32 on all host cores (the reference's nodes are torch modules too), --cpu-baseline-net-frames frames
            nparts = {}; t_net = time.perf_counter()
            for i in range(args.cpu_baseline_net_frames):
                bgr = frames[-1 - i][0]; prev = frames[-2 - i][0]
                t1 = time.perf_counter()
                V.nets.analyse_flow(lfn, prev, bgr); nparts["liteflownet_s"] = nparts.get("liteflownet_s", 0) + time.perf_counter() - t1; t1 = time.perf_counter()
                V.nets.analyse_depth(md, bgr); nparts["monodepth2_s"] = nparts.get("monodepth2_s", 0) + time.perf_counter() - t1; t1 = time.perf_counter()
                V.nets.analyse_image(mr, bgr); nparts["maskrcnn_s"] = nparts.get("maskrcnn_s", 0) + time.perf_counter() - t1
            t_net = (time.perf_counter() - t_net) / max(args.cpu_baseline_net_frames, 1)
            cpu_model = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "?")
            out["cpu_baseline"] = {"value": round(1e3 / med, 4), "unit": "frames/s", "cores": 1, "kind": "port",
                                   "sample": "SLAM stages of %d frames of the same workload on ONE pinned core (cpu %d of %d, %s): cvtColor + ORB 2000 features + frame lists, Flow2Cam on %d points, "
                                             "Flow2 on 5 x 400 object points, local BA 20 KF x 2k landmarks with the scalar C oracle (oracle/*.c, -O3) — the reference's OpenCV + g2o path as restated, "
                                             "serial like the reference library; median %.1f ms, p95 %.1f ms per frame.  The networks are NOT in `value`: see nets_all_cores / whole_chain_frames_per_s"
                                             % (len(per_frame), pin, os.cpu_count() or 0, cpu_model, n_cam_pts, med, p95),
                                   "slam_stages_1core": {"frames": len(per_frame), "median_ms": round(med, 2), "p95_ms": round(p95, 2), "mean_ms": round(float(np.mean(per_frame)), 2),
                                                         "parts_median_ms": {k: round(float(np.median(v)), 2) for k, v in parts.items()}},
                                   "nets_all_cores": {"frames": args.cpu_baseline_net_frames, "threads": nthreads, "s_per_frame": round(t_net, 3),
                                                      "parts_s": {k: round(v / max(args.cpu_baseline_net_frames, 1), 3) for k, v in nparts.items()},
                                                      "note": "torch-CPU fp32, correlation / ROI-Align / NMS / box decode = oracle C"},
                                   "whole_chain_frames_per_s": round(1.0 / (med * 1e-3 + t_net), 4) if args.cpu_baseline_net_frames else None}
        except Exception as e:
            import traceback
            out["cpu_baseline_error"] = "%s: %s" % (type(e).__name__, e); traceback.print_exc(file=sys.stderr)
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
