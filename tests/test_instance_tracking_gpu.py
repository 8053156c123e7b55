"""MI355X: what the instance label image is for.  synth.convoy_scene has five objects of one class with distinct velocities.  Detector-shaped inputs are built from its
ground truth (per object: bounding box, a 28x28 mask of ones, class 3, score by object index) and turned into the tracker's mask by the class op (the reference's sum of
class indices) and by the instance op (id base alternating 0 / 127 frame by frame, as pipeline.NetNodes does); the same System settings as test_system_gpu.py track both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAR = 3
N_FRAMES = 8
DROP_FRAME, DROP_OBJ = 5, 0            # the frame whose detector loses the highest-score object: every other detection moves up a slot


def detections(mask_gt, drop=None):
    """Ground-truth instance mask (labels 1..n) -> detector outputs in descending score order: (masks [n,1,28,28] of ones, boxes [n,4], labels [n] = CAR, object index of
    each detection).  Score by object index: object 0 first."""
    objs = [i for i in range(int(mask_gt.max())) if (mask_gt == i + 1).any() and i != drop]
    boxes = []
    for i in objs:
        ys, xs = np.nonzero(mask_gt == i + 1)
        boxes.append([xs.min(), ys.min(), xs.max(), ys.max()])
    n = len(objs)
    return torch.ones((n, 1, 28, 28)), torch.tensor(boxes, dtype=torch.float32).reshape(n, 4), torch.full((n,), CAR, dtype=torch.int64), objs


def instance_numpy(masks, boxes, labels, H, W, id_base):
    """The numpy reduction of test_instance_labels_cpu.py over nets.paste_masks (on the tensors' device): first detection in list order wins."""
    from vido_slam_amd import nets
    pasted = nets.paste_masks(masks, boxes, H, W).cpu().numpy()
    out = np.zeros((H, W), np.int32)
    for i in range(len(labels) - 1, -1, -1):
        if int(labels[i]) != 0:
            out[pasted[i]] = id_base + 1 + i
    return out


def track(vido, tmp_path, scene, frames, make_mask):
    """The clip through System.TrackRGBD with make_mask(k, ground-truth mask) as the semantic mask -> (per-frame stats, per-frame translation error, the masks)."""
    from vido_slam_amd.system import System
    from test_system_gpu import _settings
    slam = System(); slam.Init(_settings(tmp_path, scene), System.RGBD)
    stats, errs, masks, keep = [], [], [], []
    try:
        for k, (g, d, f, m) in enumerate(frames):
            mk = np.ascontiguousarray(make_mask(k, m), np.int32)
            masks.append(mk.copy())                                   # (as the detector made it: UpdateMask repaints lost labels into the array it is handed)
            args = (vido.synth.gray_to_bgr(g), np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32), mk)
            keep.append(args)
            T = slam.TrackRGBD(*args, None, None, float(k), None, len(frames))
            E = T.astype(np.float64) @ np.linalg.inv(scene.Tcw(k))
            stats.append(slam.stats()); errs.append(float(np.linalg.norm(E[:3, 3])))
    finally:
        slam.close()
    return stats, errs, masks


def test_same_class_objects_track_separately_with_instance_labels(vido, tmp_path):
    """Measured on the MI355X, n_objects per frame: class mode 0 1 1 1 1 1 1 1; instance mode 0 5 5 5 5 5 5 5; with object 0's detection dropped in frame 5 the same (the
    repaint of the lost label lands in the other id range); with the id base held at 0 that frame reports 4.  Translation error <= 0.0024 m in every run.
    The dropped-detection case asserts MORE objects than the frame's detector image holds (4): the fifth can only be UpdateMask's repaint of the lost label, tracked as a label
    of its own; and fewer with the base held at 0, where the repaint (value 1) falls onto object 1's new id.  (The System handle reports object counts, not their labels.)"""
    from vido_slam_amd import nets, pipeline
    scene = vido.synth.convoy_scene(N_FRAMES + 1)
    frames = [scene.frame(k) for k in range(N_FRAMES)]
    H, W = scene.h, scene.w
    ctx = vido.Context(width=W, height=H, max_batch=1)
    ops = nets.HipOps(ctx)
    bases = pipeline.NetNodes.ID_BASES
    assert bases == (0, 127)

    def class_mask(k, m):
        mk, bx, lb, _ = detections(m)
        return ops.mask_label_image(mk.cuda(), bx.cuda(), lb.cuda(), H, W).to(torch.int32).cpu().numpy()

    def instance_mask(drop_at=None, alternate=True):
        def make(k, m):
            mk, bx, lb, _ = detections(m, DROP_OBJ if k == drop_at else None)
            word = torch.tensor([bases[k & 1] if alternate else 0], dtype=torch.int32, device="cuda")
            return ops.mask_instance_image(mk.cuda(), bx.cuda(), lb.cuda(), H, W, id_base=word).to(torch.int32).cpu().numpy()
        return make

    # the five cars are five detections of class 3; the boxes do not overlap here, so the class image is 3 wherever any car is
    mk, bx, lb, objs = detections(frames[0][3])
    assert objs == [0, 1, 2, 3, 4]

    # class mode, the defect pinned: one label for the five cars -> at most one object (or none, if its fit fails)
    st_c, err_c, masks_c = track(vido, tmp_path, scene, frames, class_mask)
    assert set(np.unique(masks_c[-1])) == {0, CAR}
    print("class mode: n_objects per frame", [s["n_objects"] for s in st_c], "translation error", ["%.4f" % e for e in err_c])
    assert st_c[-1]["n_objects"] <= 1

    # instance mode: the objects separate; camera pose as good as with the generator's own mask (tests/test_e2e_gpu.py's bounds for this scene)
    st_i, err_i, masks_i = track(vido, tmp_path, scene, frames, instance_mask())
    for k, mk_ in enumerate(masks_i):
        for i in range(5):                                          # object i's pixels carry id base + 1 + i (all but the outermost rows / columns of its box: the 0.5 threshold of the padded mask)
            assert (mk_[frames[k][3] == i + 1] == bases[k & 1] + 1 + i).mean() > 0.9, (k, i)
        nz = np.unique(mk_[mk_ > 0])
        assert len(nz) == 5 and nz.min() == bases[k & 1] + 1 and nz.max() == bases[k & 1] + 5
    print("instance mode: n_objects per frame", [s["n_objects"] for s in st_i], "translation error", ["%.4f" % e for e in err_i])
    assert st_i[-1]["n_objects"] >= 4
    assert max(err_i) < 0.05

    # one frame loses object 0's detection and the others move up a slot.  First, on the CPU: with the base held at 0 the lost object's last id (1) IS a live id of that
    # frame (object 1's now), so UpdateMask's repaint of the lost label under its last-frame value would weld the two; with alternating bases it is not
    prev_ids = instance_numpy(*detections(frames[DROP_FRAME - 1][3])[:3], H, W, 0)
    lost_id = int(np.bincount(prev_ids[frames[DROP_FRAME - 1][3] == DROP_OBJ + 1]).argmax())
    held = instance_numpy(*detections(frames[DROP_FRAME][3], DROP_OBJ)[:3], H, W, 0)
    assert lost_id == 1 and lost_id in set(np.unique(held[held > 0]))
    assert int(np.bincount(held[frames[DROP_FRAME][3] == 2]).argmax()) == lost_id                             # it is object 1 that carries it now
    alt = instance_numpy(*detections(frames[DROP_FRAME][3], DROP_OBJ)[:3], H, W, bases[DROP_FRAME & 1])
    assert bases[(DROP_FRAME - 1) & 1] + lost_id not in set(np.unique(alt[alt > 0]))
    st_d, err_d, masks_d = track(vido, tmp_path, scene, frames, instance_mask(drop_at=DROP_FRAME))
    assert len(np.unique(masks_d[DROP_FRAME][masks_d[DROP_FRAME] > 0])) == 4                                  # the detector's image of that frame has four objects
    print("instance mode, detection of object %d dropped in frame %d: n_objects per frame" % (DROP_OBJ, DROP_FRAME), [s["n_objects"] for s in st_d],
          "translation error", ["%.4f" % e for e in err_d])
    n_detected = len(np.unique(masks_d[DROP_FRAME][masks_d[DROP_FRAME] > 0]))
    assert st_d[DROP_FRAME]["n_objects"] > n_detected                                                         # the lost object is still reported: repainted under the OTHER base's id
    assert st_d[DROP_FRAME]["n_objects"] == st_i[DROP_FRAME]["n_objects"]                                     # nothing lost against the undisturbed clip
    assert st_d[DROP_FRAME + 1]["n_objects"] >= 4 and st_d[-1]["n_objects"] >= 4
    assert max(err_d) < 0.05
    # the same clip with the base held at 0: the repaint (id 1) meets object 1's new id (shown above on the CPU) and the two are one label -> an object fewer in that frame
    st_h, _, _ = track(vido, tmp_path, scene, frames, instance_mask(drop_at=DROP_FRAME, alternate=False))
    print("the same with the id base held at 0: n_objects per frame", [s["n_objects"] for s in st_h])
    assert st_h[DROP_FRAME]["n_objects"] < st_d[DROP_FRAME]["n_objects"]
    ctx.close()


def test_netnodes_in_instance_mode_hands_over_ids_in_the_frames_range(vido):
    """NetNodes(label_mode="instance"): the detector's graph is captured with the new launch in it, and the mask's nonzero values lie in the current id base's range, two
    frames in a row (random-init weights: values only, no accuracy claim).  An unknown mode is refused at construction."""
    from vido_slam_amd import pipeline, synth, nets
    scene = synth.convoy_scene(4)
    fr = [torch.as_tensor(synth.gray_to_bgr(scene.frame(k)[0]), device="cuda") for k in range(3)]
    nodes = pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, label_mode="instance")
    assert nodes.g_det is not None, nodes.graph_error
    cap = nodes.mask_net.config.detections_per_img
    seen, painted = [], []
    for k in (1, 2):
        flow, depth, mask, labels, evs = nodes.infer(fr[k - 1], fr[k])
        for e in evs:
            torch.cuda.current_stream().wait_event(e)
        base = nodes.id_base
        mask = mask.clone(); labels = labels.clone(); n_lab = int(nodes.last_counts[0])
        torch.cuda.synchronize()
        assert mask.dtype == torch.int32 and tuple(mask.shape) == (480, 640) and tuple(labels.shape) == (cap,)
        nz = mask[mask > 0]
        print("frame %d: id base %d, %d live slots, %d labelled pixels, %d ids in the mask" % (k, base, n_lab, nz.numel(), len(torch.unique(nz))))
        assert int(nodes._id_word) == base                                                  # the word the captured kernel read
        # (random-init weights give few, mostly degenerate boxes: the image may hold a pixel or none, as the class image does; whatever it holds is in this frame's range)
        assert n_lab > 0 and bool((labels[:n_lab] > 0).all()) and bool((labels[n_lab:] == 0).all())      # live slots come first (descending score)
        if nz.numel():
            assert int(nz.min()) >= base + 1 and int(nz.max()) <= base + n_lab              # ids start above the base: labels[id - base - 1] is the id's class
        # the same frame through the eager dynamic head under the same base (the route of an overflow redo)
        img_d, lab_d = nets.analyse_image(nodes.mask_net, fr[k], feed=nodes.mask_feed, confidence=nodes.confidence, trunk=nodes.g_trunk, label_mode="instance", id_base=base)
        nzd = img_d[img_d > 0]
        assert len(lab_d) == n_lab and (nzd.numel() == 0 or (int(nzd.min()) >= base + 1 and int(nzd.max()) <= base + n_lab))
        img_c, _ = nets.analyse_image(nodes.mask_net, fr[k], feed=nodes.mask_feed, confidence=nodes.confidence, trunk=nodes.g_trunk)
        assert float(((img_c > 0) != (img_d > 0)).float().mean()) < 1e-3                    # labelled where the class image is labelled (the two kernels share the footprint)
        seen.append(base); painted.append(int(nz.numel()))
    print("labelled pixels over the two frames: %d%s" % (sum(painted), "" if sum(painted) else "  (the range check of the mask values ran EMPTY: no pixel to check)"))
    assert seen == [0, 127]
    with pytest.raises(ValueError):
        pipeline.NetNodes(vido.Context(width=640, height=480, max_batch=1), 480, 640, label_mode="instances")
