"""MI355X: the detector every Nth frame.  The facade's Mask.PropagateMissing (a frame handed over without a mask takes the previous frame's, propagated on the device:
vido_frame_propagate_mask) and pipeline.NetNodes(detect_every=N) (the detector is not launched on the frames in between; HipOps.mask_propagate warps the carried mask
through the frame's flow), with EndToEnd over such nodes.  Each GPU step runs under a time limit of its own (limit()); ONE NetNodes is built in this file."""
import contextlib
import faulthandler

import numpy as np
import pytest
import torch

N_FRAMES = 8
DETECT_ON = (0, 3, 6)


@contextlib.contextmanager
def limit(seconds, what):
    """A step that does not end within `seconds` ends the process with every thread's traceback (no waiting for a hung device)."""
    print("[step, limit %d s] %s" % (seconds, what), flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _settings_propagate(tmp_path, scene, on=True):
    from test_system_gpu import _settings
    p = _settings(tmp_path, scene)
    if on:
        with open(p, "a") as fh:
            fh.write("Mask.PropagateMissing: 1\n")
    return p


def _track(vido, settings, scene, frames, masks):
    """-> (stats per frame, translation error per frame); masks[k] None = no mask handed over"""
    from vido_slam_amd.system import System
    slam = System(); slam.Init(settings, System.RGBD)
    stats, errs, keep = [], [], []
    try:
        for k, (g, d, f, m) in enumerate(frames):
            args = (vido.synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32),
                    None if masks[k] is None else np.ascontiguousarray(masks[k], np.int32).copy())
            keep.append(args)
            T = slam.TrackRGBD(*args, None, None, float(k), None, len(frames))
            E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
            stats.append(slam.stats()); errs.append(float(np.linalg.norm(E[:3, 3])))
    finally:
        slam.close()
    return stats, errs


@pytest.mark.gpu
def test_facade_propagates_missing_masks(vido, tmp_path):
    """synth.convoy_scene, 8 frames, the true mask on frames 0, 3 and 6 and None otherwise: mask_propagated reads 0 / 1 accordingly, the last frame reports >= 4 objects and
    the translation error stays below 0.05 m on every frame (test_instance_tracking_gpu.py's bounds for this clip); printed beside the clip with the true mask on every
    frame.  Without the settings key, and on the first frame of a sequence, a missing mask is refused."""
    from vido_slam_amd.system import System
    from vido_slam_amd.host import VidoError
    scene = vido.synth.convoy_scene(N_FRAMES + 1)
    frames = [scene.frame(k) for k in range(N_FRAMES)]
    some = [frames[k][3] if k in DETECT_ON else None for k in range(N_FRAMES)]
    with limit(120, "8 frames, masks on 0 / 3 / 6"):
        st_p, err_p = _track(vido, _settings_propagate(tmp_path, scene), scene, frames, some)
    with limit(120, "8 frames, the true mask on every frame"):
        st_a, err_a = _track(vido, _settings_propagate(tmp_path, scene), scene, frames, [f[3] for f in frames])
    print("masks on 0/3/6: mask_propagated", [s["mask_propagated"] for s in st_p], "n_objects", [s["n_objects"] for s in st_p], "translation error", ["%.4f" % e for e in err_p])
    print("mask every frame: mask_propagated", [s["mask_propagated"] for s in st_a], "n_objects", [s["n_objects"] for s in st_a], "translation error", ["%.4f" % e for e in err_a])
    assert [s["mask_propagated"] for s in st_p] == [0 if k in DETECT_ON else 1 for k in range(N_FRAMES)]
    assert [s["mask_propagated"] for s in st_a] == [0] * N_FRAMES
    assert st_p[-1]["n_objects"] >= 4
    assert max(err_p) < 0.05
    g, d, f, m = frames[0]
    first = (vido.synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32))
    with limit(60, "refusals: first frame without a mask; key at 0"):
        slam = System(); slam.Init(_settings_propagate(tmp_path, scene), System.RGBD)
        try:
            with pytest.raises(VidoError):
                slam.TrackRGBD(*first, None, None, None, 0.0, None, 4)
        finally:
            slam.close()
        slam = System(); slam.Init(_settings_propagate(tmp_path, scene, on=False), System.RGBD)
        try:
            slam.TrackRGBD(first[0], first[1].copy(), first[2], np.ascontiguousarray(m, np.int32), None, None, 0.0, None, 4)
            with pytest.raises(VidoError):
                slam.TrackRGBD(first[0], first[1].copy(), first[2], None, None, None, 1.0, None, 4)
            assert slam.stats()["mask_propagated"] == 0
        finally:
            slam.close()


@pytest.mark.gpu
def test_netnodes_detect_every_and_end_to_end(vido, tmp_path):
    """NetNodes(detect_every=3, label_mode="instance") at 480 x 640, 7 frames: 3 detector runs, the frames in between propagated, the id base held over them; on one
    propagated frame a blob image written into carried_mask comes back as HipOps.mask_propagate of it through the returned flow, bit for bit; then 6 frames of EndToEnd
    over the same nodes: 2 more detector runs, no error.  (Random-init networks: the flow is whatever LiteFlowNet makes of the pair; what is pinned is the plumbing.)"""
    from vido_slam_amd import pipeline
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    from test_mask_propagate_gpu import blob_image
    scene = vido.synth.convoy_scene(N_FRAMES)
    frames = [scene.frame(k) for k in range(7)]
    with limit(600, "building NetNodes(detect_every=3, label_mode='instance')"):
        nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, label_mode="instance", detect_every=3)
        torch.cuda.synchronize()
    assert nodes.g_det is not None, nodes.graph_error
    assert nodes.detect_every == 3 and nodes.detector_runs == 0 and tuple(nodes.carried_mask.shape) == (480, 640) and nodes.carried_mask.dtype == torch.int32
    fr = [torch.as_tensor(vido.synth.gray_to_bgr(f[0]), device="cuda") for f in frames]
    blob = torch.as_tensor(blob_image(480, 640, 5, labels=(1, 2, 130, 254))).cuda()
    propagated, bases = [], []
    with limit(120, "7 frames through infer()"):
        for k in range(7):
            if k == 4:
                nodes.carried_mask.copy_(blob)                                # an external detector's image: the next propagated frame starts from it
            flow, depth, mask, labels, evs = nodes.infer(fr[max(k - 1, 0)], fr[k])
            for e in evs:
                torch.cuda.current_stream().wait_event(e)
            propagated.append(nodes.last_propagated); bases.append(nodes.id_base)
            assert mask.dtype == torch.int32 and tuple(mask.shape) == (480, 640)
            if nodes.last_propagated:
                assert mask.data_ptr() == nodes.carried_mask.data_ptr() and int(nodes.last_counts[1]) == 0      # no detections reported: nothing to redo
            if k == 4:
                expect = nodes.ops.mask_propagate(blob, flow)
                torch.cuda.synchronize()
                print("frame 4: %d labelled pixels in the blob image, %d after the propagation; |flow| max %.2f" % (int((blob > 0).sum()), int((mask > 0).sum()), float(flow.abs().max())))
                assert torch.equal(mask, expect) and int((mask > 0).sum()) > 0
        torch.cuda.synchronize()
    assert propagated == [False, True, True, False, True, True, False]
    assert bases == [0, 0, 0, 127, 127, 127, 0]
    assert nodes.detector_runs == 3 and nodes.propagated_frames == 4
    runs0 = nodes.detector_runs
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    e2e = pipeline.EndToEnd(nodes, slam, n_image=10 ** 6, feed="given")
    try:
        with limit(180, "6 frames of EndToEnd over the same nodes"):
            for k in range(6):
                g, d, f, m = frames[k]
                e2e.push(vido.synth.gray_to_bgr(g), (np.ascontiguousarray(d, np.float32), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32)))
            e2e.finish()
    finally:
        e2e.close(); slam.close()
    assert e2e.err is None and len(e2e.poses) == 6
    assert nodes.detector_runs == runs0 + 2                                   # calls 7 .. 12 of the nodes: the detector runs on 9 and 12


def test_detect_every_argument_checks():
    """Refused before any network is built (no GPU needed: the checks come first)."""
    from vido_slam_amd import pipeline
    for bad in (0, 2.5, -1, True, "2"):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, detect_every=bad)
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, detect_every=2, on_range="recompute")
