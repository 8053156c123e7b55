"""MI355X: vido_mask_instance_image (csrc/nets.hip::k_paste_instance) bit for bit against the first-covering-detection reduction over nets.paste_masks (the yardstick
test_maskrcnn_gpu.py uses for the class-sum kernel), its area counters, its id base through a device word, its footprint against vido_mask_label_image, its argument
checks, and its replay inside a captured graph."""
import ctypes as C
import numpy as np
import pytest
import torch
from vido_slam_amd import nets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


def reference(masks, boxes, labels, H, W, id_base=0):
    """numpy: id_base + 1 + index of the first detection (list order) with a nonzero class whose pasted mask (nets.paste_masks, bool [n,H,W]) covers the pixel; 0 if none."""
    pasted = nets.paste_masks(masks, boxes, H, W).cpu().numpy()
    lab = labels.cpu().numpy()
    out = np.zeros((H, W), np.int64)
    for i in range(len(lab) - 1, -1, -1):                           # painted from the last to the first: the first one ends on top
        if lab[i] != 0:
            out[pasted[i]] = id_base + 1 + i
    return out.astype(np.uint8)


def clustered(rng, n, H, W):
    """n detections on 8 cluster centres (heavy mutual overlap, some boxes across the image border), M = 28 soft masks in (0, 1) with entries exactly 0.5, some class-0 slots."""
    cen = np.stack([rng.uniform(0.1 * W, 0.9 * W, 8), rng.uniform(0.1 * H, 0.9 * H, 8)], 1)
    c = cen[rng.randint(0, 8, n)] + rng.normal(0, 12, (n, 2)); wh = rng.uniform(20, 0.45 * H, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    m = rng.uniform(0.02, 0.98, (n, 1, 28, 28)).astype(np.float32)
    m[rng.rand(n, 1, 28, 28) < 0.1] = 0.5
    labels = rng.randint(1, 81, n).astype(np.int64)
    if n > 4:
        labels[rng.choice(n, n // 10, replace=False)] = 0
    return torch.from_numpy(m).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(labels).cuda()


@pytest.mark.parametrize("H,W", [(480, 640), (375, 1242)])
@pytest.mark.parametrize("n", [0, 1, 100, 127])
def test_instance_image_equals_the_first_hit_reduction_over_paste_masks(ctx, H, W, n):
    ops = nets.HipOps(ctx)
    masks, boxes, labels = clustered(np.random.RandomState(n + H), n, H, W)
    for base in (0, 127):
        word = torch.tensor([base], dtype=torch.int32, device="cuda")
        img, area = ops.mask_instance_image(masks, boxes, labels, H, W, id_base=word, areas=True)
        ref = reference(masks, boxes, labels, H, W, base)
        got = img.cpu().numpy()
        print("n %d %dx%d base %d: %d of %d pixels differ, %d labelled" % (n, H, W, base, int((got != ref).sum()), H * W, int((ref > 0).sum())))
        assert got.dtype == np.uint8 and np.array_equal(got, ref)
        if n >= 100:
            assert (ref > 0).mean() > 0.2 and len(np.unique(ref)) > n // 3                 # the case is what it says: a well covered image, many owners
        counts = np.bincount(got.ravel(), minlength=256)
        assert np.array_equal(area.cpu().numpy(), counts[base + 1:base + 1 + n])            # pixels per detection; class-0 slots own none
        assert torch.equal(ops.mask_instance_image(masks, boxes, labels, H, W, id_base=word), img)      # without the counters: the same image
        if base:
            assert torch.equal(ops.mask_instance_image(masks, boxes, labels, H, W, id_base=base), img)  # the base as a host value


def test_footprint_is_the_class_kernels(ctx):
    """No overlap, every class = c: class image == c * (instance image > 0) — both kernels cover the same pixels for every detection (soft masks, boxes across the border)."""
    ops = nets.HipOps(ctx)
    rng = np.random.RandomState(11)
    H, W, c = 480, 640, 3
    gx, gy = np.meshgrid(np.arange(10), np.arange(6))
    org = np.stack([gx.ravel() * 64 - 12.0, gy.ravel() * 80 - 14.0], 1)                     # a 10 x 6 grid of 64 x 80 cells, the first row and column cut by the border
    wh = rng.uniform(16, 44, (60, 2)); off = 6.0 + rng.uniform(0, 1, (60, 2)) * (np.array([52.0, 68.0]) - wh)
    # a box lies in [6, 58] x [6, 74] of its cell; pasting widens it by 30/28 about its centre and truncation adds a pixel: inside (3.4, 60.6) x (3.4, 76.6), disjoint
    boxes = torch.from_numpy(np.concatenate([org + off, org + off + wh], 1).astype(np.float32)).cuda()
    m = rng.uniform(0.02, 0.98, (60, 1, 28, 28)).astype(np.float32); m[rng.rand(60, 1, 28, 28) < 0.1] = 0.5
    masks = torch.from_numpy(m).cuda(); labels = torch.full((60,), c, dtype=torch.int64, device="cuda")
    assert int(nets.paste_masks(masks, boxes, H, W).sum(0).max()) == 1
    inst = ops.mask_instance_image(masks, boxes, labels, H, W)
    cls = ops.mask_label_image(masks, boxes, labels, H, W)
    assert int((inst > 0).sum()) > 10000 and torch.equal(cls, (inst > 0).to(torch.uint8) * c)
    assert len(torch.unique(inst)) == 61


def test_bad_arguments_return_the_error_code_and_leave_the_context_usable(vido, ctx):
    ops = nets.HipOps(ctx)
    lib, h = ctx.lib, ctx.h
    H, W = 64, 96
    masks, boxes, labels = clustered(np.random.RandomState(2), 256, H, W)
    out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda m, b, l, n, o, Hh=H: lib.vido_mask_instance_image(h, m, b, l, n, 28, 1, C.c_float(0.5), Hh, W, None, o, None)
    assert call(p(masks), p(boxes), p(labels), 256, p(out)) == -4                            # VIDO_E_CAPACITY: 256 ids do not fit u8
    assert b"255" in lib.vido_last_error(h)
    assert call(p(masks), p(boxes), p(labels), -1, p(out)) == -1                             # VIDO_E_INVALID
    assert call(None, p(boxes), p(labels), 5, p(out)) == -1 and call(p(masks), None, p(labels), 5, p(out)) == -1 and call(p(masks), p(boxes), None, 5, p(out)) == -1
    assert call(p(masks), p(boxes), p(labels), 5, None) == -1 and call(p(masks), p(boxes), p(labels), 5, p(out), 0) == -1
    torch.cuda.synchronize()
    assert not out.any()                                                                     # nothing was launched
    with pytest.raises(vido.VidoError) as e:
        ops.mask_instance_image(masks[:129], boxes[:129], labels[:129], H, W, id_base=127)   # host-known base: 129 + 127 > 255
    assert e.value.code == -4
    with pytest.raises(vido.VidoError):
        ops.mask_instance_image(masks, boxes, labels, H, W)
    got = ops.mask_instance_image(masks[:128], boxes[:128], labels[:128], H, W, id_base=127)  # 128 + 127 = 255 fits; the context still works
    assert np.array_equal(got.cpu().numpy(), reference(masks[:128], boxes[:128], labels[:128], H, W, 127))


def test_replay_inside_a_captured_graph_follows_inputs_and_the_id_word(ctx):
    ops = nets.HipOps(ctx)
    H, W, n = 480, 640, 100
    word = torch.zeros((1,), dtype=torch.int32, device="cuda")
    fn = lambda m, b, l: ops.mask_instance_image(m, b, l, H, W, id_base=word, areas=True)
    a = clustered(np.random.RandomState(21), n, H, W)
    g = nets.Graphed(fn, list(a))
    for seed, base in ((21, 0), (22, 127), (23, 0)):
        m, b, l = clustered(np.random.RandomState(seed), n, H, W)
        word.fill_(base)                                                                     # in stream order before the replay, as NetNodes does
        img_g, area_g = [t.clone() for t in g(m, b, l)]
        img_e, area_e = fn(m, b, l)
        torch.cuda.synchronize()
        assert torch.equal(img_g, img_e) and torch.equal(area_g, area_e)
        assert np.array_equal(img_g.cpu().numpy(), reference(m, b, l, H, W, base))
        nz = img_g[img_g > 0]
        assert int(nz.min()) > base and int(nz.max()) <= base + n
