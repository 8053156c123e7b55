"""No GPU: the torch tail of nets.analyse_image (nets.label_image_torch) in instance mode on CPU tensors, against a numpy loop over nets.paste_masks written here:
the first detection in descending score order that covers a pixel owns it.  Integers only, exact equality."""
import numpy as np
import pytest
import torch
from vido_slam_amd import nets

H, W = 60, 80


def instance_reference(pasted, labels, id_base=0):
    """pasted: bool [n,H,W] in priority order, labels [n] -> u8 [H,W]: id_base + 1 + index of the first covering detection with a nonzero class, 0 if none."""
    n, h, w = pasted.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            for i in range(n):
                if labels[i] != 0 and pasted[i, y, x]:
                    out[y, x] = id_base + 1 + i
                    break
    return out


def class_reference(pasted, labels):
    out = np.zeros(pasted.shape[1:], np.uint8)
    for i in range(len(labels)):                                   # run_mask_rcnn.py:112-118: blank_mask += mask * class_index, in u8
        out += (pasted[i] * labels[i]).astype(np.uint8)
    return out


def run(boxes, scores, labels, masks=None, confidence=0.8, id_base=0, seed=0):
    """Both modes of the tail and both references for detections given in ARBITRARY order; the references see them sorted by score, as select_top_predictions does."""
    n = len(boxes)
    g = torch.Generator().manual_seed(seed)
    masks = torch.rand((n, 1, 28, 28), generator=g) * 0.6 + 0.4 if masks is None else masks            # mostly above the threshold, ragged edges
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(n, 4); scores = torch.tensor(scores, dtype=torch.float32); labels = torch.tensor(labels, dtype=torch.int64)
    order = [i for i in np.argsort(-scores.numpy(), kind="stable") if scores[i] > confidence]
    pasted = nets.paste_masks(masks[order], boxes[order], H, W).numpy()
    lab = labels.numpy()[order]
    img_i, lab_i = nets.label_image_torch(masks, boxes, scores, labels, H, W, confidence, "instance", id_base)
    img_c, lab_c = nets.label_image_torch(masks, boxes, scores, labels, H, W, confidence, "class")
    assert img_i.dtype == torch.uint8 and tuple(img_i.shape) == (H, W)
    assert np.array_equal(lab_i.numpy(), lab) and np.array_equal(lab_c.numpy(), lab)
    ref_i = instance_reference(pasted, lab, id_base)
    assert np.array_equal(img_i.numpy(), ref_i)
    assert np.array_equal(img_c.numpy(), class_reference(pasted, lab))
    return img_i.numpy(), img_c.numpy(), pasted, lab


def test_disjoint_masks_get_one_id_each():
    img, cls, pasted, lab = run([[2, 3, 20, 25], [30, 5, 55, 30], [10, 35, 70, 55]], [0.95, 0.99, 0.9], [3, 3, 1])
    assert not (pasted.sum(0) > 1).any()
    assert set(np.unique(img)) == {0, 1, 2, 3}
    assert (cls[img == 1] == 3).all() and (cls[img == 2] == 3).all() and (cls[img == 3] == 1).all()      # labels[id - 1] is the class
    for i in range(3):
        assert np.array_equal(img == i + 1, pasted[i])


def test_same_class_overlap_goes_to_the_higher_score_never_a_sum():
    ones = torch.ones((2, 1, 28, 28))
    img, cls, pasted, lab = run([[5, 5, 40, 40], [25, 20, 70, 50]], [0.85, 0.97], [3, 3], masks=ones)      # the second detection has the higher score -> id 1
    both = pasted[0] & pasted[1]
    assert both.sum() > 100
    assert (img[both] == 1).all() and (cls[both] == 6).all()                      # class mode: car + car = 6 ("bus"); instance mode: the higher score's id
    assert set(np.unique(img)) == {0, 1, 2}
    assert np.array_equal(img == 2, pasted[1] & ~pasted[0])


def test_different_class_overlap_is_not_the_sum_of_the_classes():
    ones = torch.ones((2, 1, 28, 28))
    a, b = 1, 3
    img, cls, pasted, lab = run([[10, 10, 50, 45], [30, 20, 75, 55]], [0.99, 0.9], [a, b], masks=ones)
    both = pasted[0] & pasted[1]
    assert both.sum() > 100 and (cls[both] == a + b).all()
    assert (img[both] == 1).all() and int(lab[0]) == a
    assert not np.isin(img, [a + b]).any()


def test_box_partly_outside_the_image():
    img, cls, pasted, lab = run([[-15, -10, 20, 18], [60, 40, 100, 75], [-5, 50, 12, 70]], [0.9, 0.95, 0.99], [2, 2, 2])
    assert img[0, 0] == 3 and img[H - 1, W - 1] == 2 and img[H - 1, 0] == 1            # ids by descending score: 0.99 -> 1, 0.95 -> 2, 0.9 -> 3


def test_no_detection_gives_an_empty_image():
    img, cls, pasted, lab = run(np.zeros((0, 4)), [], [])
    assert not img.any() and not cls.any() and len(lab) == 0
    img, cls, pasted, lab = run([[5, 5, 40, 40]], [0.5], [3])                     # below the confidence: not kept
    assert not img.any() and len(lab) == 0


def test_class_zero_slot_is_skipped_and_keeps_its_id():
    ones = torch.ones((3, 1, 28, 28))
    img, cls, pasted, lab = run([[5, 5, 30, 30], [20, 20, 50, 50], [40, 35, 75, 55]], [0.99, 0.95, 0.9], [3, 0, 3], masks=ones)
    assert list(lab) == [3, 0, 3]
    assert set(np.unique(img)) == {0, 1, 3}                                       # id 2 belongs to the class-0 slot: never painted, ids after it not shifted
    assert np.array_equal(img == 3, pasted[2])                                    # incl. where the skipped slot's mask lies over it
    assert (pasted[1] & pasted[2]).any() and not img[pasted[1] & ~pasted[0] & ~pasted[2]].any()


def test_id_base_shifts_the_ids_and_the_range_is_checked():
    img0, _, pasted, _ = run([[2, 3, 20, 25], [15, 5, 55, 30]], [0.95, 0.99], [3, 3])
    img1, _, _, _ = run([[2, 3, 20, 25], [15, 5, 55, 30]], [0.95, 0.99], [3, 3], id_base=127)
    assert np.array_equal(img1, np.where(img0 > 0, img0.astype(np.int32) + 127, 0).astype(np.uint8)) and img1.max() == 129
    t = torch.tensor([127], dtype=torch.int32)                                    # the base as a one-element tensor, as the pipeline holds it
    boxes = torch.tensor([[2.0, 3, 20, 25], [15, 5, 55, 30]]); masks = torch.rand((2, 1, 28, 28), generator=torch.Generator().manual_seed(0)) * 0.6 + 0.4
    img2, _ = nets.label_image_torch(masks, boxes, torch.tensor([0.95, 0.99]), torch.tensor([3, 3]), H, W, 0.8, "instance", t)
    assert np.array_equal(img2.numpy(), img1)
    with pytest.raises(ValueError):
        nets.label_image_torch(masks, boxes, torch.tensor([0.95, 0.99]), torch.tensor([3, 3]), H, W, 0.8, "instance", 254)
    with pytest.raises(ValueError):
        nets.label_image_torch(masks, boxes, torch.tensor([0.95, 0.99]), torch.tensor([3, 3]), H, W, 0.8, "instances")


def test_max_instances_keeps_the_highest_scores_and_drops_the_rest_from_image_and_labels():
    """What NetNodes asks of an overflow redo (more detections than an id range holds): the sequence goes on with the top of the list."""
    boxes = torch.tensor([[2.0, 3, 20, 25], [15, 5, 55, 30], [30, 30, 70, 55], [5, 35, 40, 58], [50, 2, 78, 20]])
    scores = torch.tensor([0.85, 0.99, 0.9, 0.95, 0.81]); labels = torch.tensor([3, 3, 1, 3, 2]); masks = torch.ones((5, 1, 28, 28))
    full, lab_full = nets.label_image_torch(masks, boxes, scores, labels, H, W, 0.8, "instance", 127)
    img, lab = nets.label_image_torch(masks, boxes, scores, labels, H, W, 0.8, "instance", 127, max_instances=3)
    assert lab.tolist() == lab_full.tolist()[:3] == [3, 3, 1]
    order = [1, 3, 2]                                                             # the three highest scores
    ref = instance_reference(nets.paste_masks(masks[order], boxes[order], H, W).numpy(), lab.numpy(), 127)
    assert np.array_equal(img.numpy(), ref) and set(np.unique(img.numpy())) == {0, 128, 129, 130}
    assert np.array_equal(img.numpy(), np.where(full.numpy() <= 130, full.numpy(), 0))       # (the dropped detections rank below the kept ones: leaving them out frees no pixel)
    cls, lab_c = nets.label_image_torch(masks, boxes, scores, labels, H, W, 0.8, "class", 0, max_instances=3)
    assert len(lab_c) == 5                                                        # class mode is not touched by it


def test_many_random_overlapping_detections():
    rng = np.random.RandomState(3)
    n = 40
    xy = rng.uniform(-10, 60, (n, 2)); wh = rng.uniform(4, 40, (n, 2))
    labels = rng.randint(0, 5, n)
    g = torch.Generator().manual_seed(9)
    masks = torch.rand((n, 1, 28, 28), generator=g)
    run(np.concatenate([xy, xy + wh], 1), rng.uniform(0.7, 1.0, n), labels, masks=masks, seed=1)
    run(np.concatenate([xy, xy + wh], 1), rng.uniform(0.7, 1.0, n), labels, masks=masks, id_base=127)
