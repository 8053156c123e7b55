"""MI355X: what the connected-component op is for.  synth.convoy_scene has five objects of ONE class; its class image 3 * (gt > 0) is what the reference's node or a dataset's
semantic mask hands over, and through it the tracker sees one label for the five cars (test_instance_tracking_gpu.py pins that at n_objects <= 1).
(a) pipeline.InstanceIds.from_classes gives each car one persistent id from the class image alone; (b) - (d) the facade's settings key Mask.SplitInstances: 1 splits the
frame's mask inside the tracker (vido_frame_split_mask), with every frame's mask, with masks on frames 0 / 3 / 6 and Mask.PropagateMissing: 1, and on device buffers
adopted zero-copy.  The networks never run."""
import numpy as np
import pytest
import torch

from test_instance_tracking_gpu import track, CAR, N_FRAMES
from test_detect_every_gpu import limit, DETECT_ON

pytestmark = pytest.mark.gpu

CLIP = {}


def clip(vido):
    """-> scene, frames, the class image of every frame (3 wherever any car is).  Made once, never modified."""
    if not CLIP:
        scene = vido.synth.convoy_scene(N_FRAMES + 1)
        frames = [scene.frame(k) for k in range(N_FRAMES)]
        cls = [(CAR * (f[3] > 0)).astype(np.int32) for f in frames]
        for c in cls:
            c.setflags(write=False)
        CLIP.update(scene=scene, frames=frames, cls=cls)
    return CLIP


def settings(tmp_path, scene, *lines):
    from test_system_gpu import _settings
    p = _settings(tmp_path, scene)
    with open(p, "a") as fh:
        for ln in lines:
            fh.write(ln + "\n")
    return p


def run_clip(vido, path, scene, frames, masks):
    """test_instance_tracking_gpu.py's track() with a mask of None allowed and the split counters read -> (stats, translation errors, split counters) per frame; the
    mask arrays handed over are checked to come back untouched."""
    from vido_slam_amd.system import System
    slam = System(); slam.Init(path, System.RGBD)
    stats, errs, split, keep = [], [], [], []
    try:
        for k, (g, d, f, m) in enumerate(frames):
            mk = None if masks[k] is None else np.ascontiguousarray(masks[k], np.int32).copy()
            args = (vido.synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32), mk)
            keep.append(args)
            T = slam.TrackRGBD(*args, None, None, float(k), None, len(frames))
            E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
            stats.append(slam.stats()); errs.append(float(np.linalg.norm(E[:3, 3]))); split.append(slam.mask_split_stats())
        for k, a in enumerate(keep):
            assert masks[k] is None or np.array_equal(a[3], masks[k]), "the caller's mask of frame %d was written" % k
    finally:
        slam.close()
    return stats, errs, split


def test_from_classes_gives_each_car_one_id(vido):
    """(a) InstanceIds.from_classes on the class image over 8 frames with the scene's flow: five ids, each object's dominant id over its true pixels is one value for all
    frames, the table reads class 3 for exactly those ids; a min_area above every car leaves the image empty."""
    from vido_slam_amd import nets, pipeline
    c = clip(vido)
    frames, H, W = c["frames"], c["scene"].h, c["scene"].w
    ctx = vido.Context(width=W, height=H, max_batch=1)
    ids = pipeline.InstanceIds(nets.HipOps(ctx), H, W, hold=0)
    dom = []
    for k in range(N_FRAMES):
        flow = None if k == 0 else torch.from_numpy(np.ascontiguousarray(frames[k - 1][2], np.float32)).cuda()
        m = ids.from_classes(torch.from_numpy(c["cls"][k].copy()).cuda(), flow)
        assert m.data_ptr() == ids.mask.data_ptr()
        mk = m.cpu().numpy()
        assert ids.split_stats.cpu().tolist() == [5, 0, 0, 5]
        assert np.array_equal(mk > 0, c["cls"][k] > 0)
        dom.append([int(np.bincount(mk[frames[k][3] == i + 1]).argmax()) for i in range(5)])
        assert all((mk[frames[k][3] == i + 1] == dom[-1][i]).all() for i in range(5))          # a component is one object, whole
        table = ids.classes_by_id.cpu().numpy()
        assert sorted((np.nonzero(table)[0] + 1).tolist()) == sorted(dom[-1]) and set(table[table != 0].tolist()) == {CAR}
    print("dominant id per object, frame by frame:", dom, "counters of the last association:", ids.stats.cpu().tolist())
    assert len(set(dom[0])) == 5 and min(dom[0]) > 0
    for i in range(5):
        assert len({d[i] for d in dom}) == 1, (i, [d[i] for d in dom])
    assert ids.stats.cpu().tolist() == [5, 0, 0, 0]                   # the last frame: five matches, nothing fresh, lost or left out
    m = ids.from_classes(torch.from_numpy(c["cls"][0].copy()).cuda(), None, min_area=20000)
    assert not m.any().item() and ids.split_stats.cpu().tolist() == [5, 5, 0, 0]
    torch.cuda.synchronize()
    ctx.close()


def test_class_image_tracks_five_objects_with_split_instances(vido, tmp_path, monkeypatch):
    """(b) test_instance_tracking_gpu.py's track() on the class image 3 * (gt > 0), settings of test_system_gpu._settings plus Mask.SplitInstances: 1: n_objects >= 4 on the
    last frame and translation error < 0.05 on every frame (that file's bounds for its instance mode).  Without the key the same clip reports n_objects <= 1 (that file's
    class mode; a build that ignores the key fails here)."""
    import test_system_gpu
    c = clip(vido)
    plain = test_system_gpu._settings

    def with_key(tmp, scene, rgb=0):
        p = plain(tmp, scene, rgb)
        with open(p, "a") as fh:
            fh.write("Mask.SplitInstances: 1\n")
        return p
    monkeypatch.setattr(test_system_gpu, "_settings", with_key)
    with limit(120, "8 frames, class image, Mask.SplitInstances: 1"):
        st, err, masks = track(vido, tmp_path, c["scene"], c["frames"], lambda k, m: c["cls"][k])
    print("Mask.SplitInstances: 1: n_objects per frame", [s["n_objects"] for s in st], "translation error", ["%.4f" % e for e in err])
    assert set(np.unique(masks[-1])) == {0, CAR}                      # what was handed over is the class image
    assert st[-1]["n_objects"] >= 4
    assert max(err) < 0.05


def test_split_with_masks_on_some_frames_and_the_counters(vido, tmp_path):
    """(c) a mask on frames 0 / 3 / 6 only, Mask.PropagateMissing: 1 and Mask.SplitInstances: 1: n_objects >= 4 on the last frame.  (d) mask_split_stats() reads kept == 5
    on a split frame and zeros on a propagated one; Mask.MinInstanceArea at the median car drops the smaller ones; with the key at 0 the counters stay zero."""
    c = clip(vido)
    scene, frames = c["scene"], c["frames"]
    some = [c["cls"][k] if k in DETECT_ON else None for k in range(N_FRAMES)]
    with limit(120, "8 frames, class image on 0 / 3 / 6, both keys"):
        st, err, split = run_clip(vido, settings(tmp_path, scene, "Mask.PropagateMissing: 1", "Mask.SplitInstances: 1"), scene, frames, some)
    print("masks on 0/3/6: n_objects", [s["n_objects"] for s in st], "split counters", split, "translation error", ["%.4f" % e for e in err])
    assert [s["mask_propagated"] for s in st] == [0 if k in DETECT_ON else 1 for k in range(N_FRAMES)]
    assert [sp for sp in split] == [(5, 0, 0, 5) if k in DETECT_ON else (0, 0, 0, 0) for k in range(N_FRAMES)]
    assert st[-1]["n_objects"] >= 4
    assert max(err) < 0.05
    areas = sorted(int((frames[0][3] == i + 1).sum()) for i in range(5))
    cut = areas[2]                                                    # the median car of frame 0: the smaller ones go
    gone = sum(a < cut for a in areas)
    assert 1 <= gone <= 2
    with limit(60, "2 frames, Mask.MinInstanceArea"):
        _, _, split = run_clip(vido, settings(tmp_path, scene, "Mask.SplitInstances: 1", "Mask.MinInstanceArea: %d" % cut), scene, frames[:2], c["cls"][:2])
    assert split[0] == (5, gone, 0, 5 - gone), (split, areas, cut)
    with limit(60, "2 frames, the key at 0"):
        st0, _, split = run_clip(vido, settings(tmp_path, scene, "Mask.SplitInstances: 0"), scene, frames[:3], c["cls"][:3])
    assert split == [(0, 0, 0, 0)] * 3 and st0[-1]["n_objects"] <= 1


def test_device_form_with_adopted_buffers_leaves_the_callers_mask(vido, tmp_path):
    """TrackRGBDDevice with zero-copy maps and Mask.SplitInstances: 1: the slot adopts a tracker-owned buffer that holds the split image; the caller's device mask reads the
    class image afterwards, the counters read kept == 5 on every frame, n_objects >= 4 on the last frame.  The same without zero-copy maps (the slot's own copy is split)."""
    from vido_slam_amd.system import System
    c = clip(vido)
    scene, frames = c["scene"], c["frames"]
    H, W = scene.h, scene.w
    for zero_copy in (True, False):
        slam = System(); slam.Init(settings(tmp_path, scene, "Mask.SplitInstances: 1"), System.RGBD)
        slam.SetZeroCopyMaps(zero_copy)
        keep, nobj, split = [], [], []
        try:
            with limit(120, "8 frames on device buffers, zero-copy maps %s" % zero_copy):
                for k, (g, d, f, m) in enumerate(frames):
                    bufs = (torch.from_numpy(vido.synth.gray_to_bgr(g)).cuda(), torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda(), torch.from_numpy(c["cls"][k].copy()).cuda())
                    keep.append(bufs)
                    torch.cuda.synchronize()
                    slam.TrackRGBDDevice(bufs[0].data_ptr(), 3, W, H, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), None, float(k), len(frames))
                    nobj.append(slam.stats()["n_objects"]); split.append(slam.mask_split_stats())
                    assert np.array_equal(bufs[3].cpu().numpy(), c["cls"][k]), "the caller's device mask of frame %d was written" % k
        finally:
            slam.SetZeroCopyMaps(False)                               # (the switch is the process's, not the handle's)
            slam.close()
        print("device form, zero-copy maps %s: n_objects" % zero_copy, nobj, "split counters", split)
        assert split == [(5, 0, 0, 5)] * N_FRAMES
        assert nobj[-1] >= 4
