"""The static mask head on the LIVE slots only: the `_n` entry points of its four kernels (a device-side count, read when the kernel runs; csrc/conv3x3h.hip, csrc/conv1x1.hip
RES 3, csrc/nets.hip) and analyse_image_static, which orders the slots first and hands the mask head the count.

The properties, per kernel: the live rows are bit for bit those of the uncounted call; the dead rows of the OUTPUT are not written (a sentinel stays; the logit kernel writes
zeros instead); the dead rows of the INPUT are not read — they hold NaN, infinity and 70000 here, like the stale bytes of a torch.empty would, and the split-fp16 range flag
stays down.  Nothing here provokes a fault: the hostile values are data in rows that must not be read."""
import ctypes as C
import os
import numpy as np
import pytest
import torch
from vido_slam_amd import nets

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "maskrcnn_graph.npz"))
TINY = nets.MaskRCNNConfig(blocks=(3, 4, 6, 3), groups=4, width_per_group=4, res2_out=32, stem_out=16, fpn_out=16, mlp_dim=64, num_classes=7,
                           mask_layers=(16, 16, 16, 16), detections_per_img=20)
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ops(ctx):
    return nets.HipOps(ctx)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _hostile_(x, live):
    """rows live .. of x: what a stale buffer may hold"""
    if live < x.shape[0]:
        x[live:] = float("nan")
        flat = x[live:].reshape(x.shape[0] - live, -1)
        flat[:, 1::3] = float("inf"); flat[:, 2::3] = 70000.0
    return x


def _counts(n):
    return ((0, 0), (1, 1), (3, min(3, n)), (n, n), (n + 5, n), (-2, 0))              # (the word, the live rows it means: clamped to [0, n])


def _conv3x3_n(ops, x, wp, b, y, cout, slope, word):
    n, cin, h, w = x.shape
    ops._adopt_stream()
    ops.ctx._check(ops.ctx.lib.vido_conv3x3_h_bias_act_n(ops.ctx.h, _p(x), _p(wp), _p(b), _p(y), n, cin, cout, h, w, C.c_float(slope), _p(word)))


@pytest.mark.parametrize("n,cin,cout", [(6, 16, 128), (200, 16, 128), (4, 256, 256)])
def test_conv3x3_h_with_a_live_count(ops, n, cin, cout):
    """n = 6 takes the 8-row form, n = 200 the 16-row form (200 blocks >= the kernel's threshold of 190), n = 4 has the mask head's real channel counts."""
    from vido_slam_amd.nets.ops import pack_conv3x3_h
    H = W = 14
    lib = ops.ctx.lib
    assert (lib.vido_conv3x3_h_workgroups(n, cout, H, W) == n * (cout // 128)) == (n == 200)                  # 16-row blocks: one per image and channel tile; 8-row: two
    g = torch.Generator().manual_seed(n + cin)
    x = torch.randn(n, cin, H, W, generator=g).cuda()
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5); b = torch.randn(cout, generator=g).cuda()
    wp = pack_conv3x3_h(w).cuda()
    full = ops.conv3x3_h_bias_act(x, wp, b, cout, 0.0)
    torch.cuda.synchronize(); assert ops.conv1x1_range_flag() == 0
    for word, live in _counts(n):
        xh = _hostile_(x.clone(), live)
        y = torch.full((n, cout, H, W), SENTINEL, device="cuda")
        _conv3x3_n(ops, xh, wp, b, y, cout, 0.0, _word(word))
        torch.cuda.synchronize()
        assert ops.conv1x1_range_flag() == 0, (word, "a dead row was read")
        assert torch.equal(y[:live], full[:live]), word
        assert bool((y[live:] == SENTINEL).all()), word
    # the plain entry point and a NULL count: every image
    y = torch.full((n, cout, H, W), SENTINEL, device="cuda")
    _conv3x3_n(ops, x, wp, b, y, cout, 0.0, None)
    assert torch.equal(y, full)
    assert torch.equal(ops.conv3x3_h_bias_act(x, wp, b, cout, 0.0, _word(n)), full)


def test_roi_align_fpn_nhwc_with_a_live_count(ops):
    n, Cc, res = 9, 80, 14                                                             # (80 channels: a full 64-channel group and a ragged one)
    rng = np.random.RandomState(3)
    feats = [torch.randn(1, Cc, 24 >> l, 32 >> l, device="cuda") for l in range(4)]
    nh = [ops.to_nhwc(f) for f in feats]
    scales = (0.25, 0.125, 0.0625, 0.03125)
    xy = rng.uniform(-10, 90, (n, 2)); wh = rng.uniform(2, 70, (n, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).cuda()
    lvl = torch.from_numpy((np.arange(n) % 4).astype(np.int32)).cuda()
    full = ops.roi_align_fpn_nhwc(nh, boxes, lvl, (res, res), scales, 2)
    fp = (C.c_void_p * 4)(*[f.data_ptr() for f in nh]); Hs = (C.c_int * 4)(*[f.shape[1] for f in nh]); Ws = (C.c_int * 4)(*[f.shape[2] for f in nh]); sc = (C.c_float * 4)(*scales)
    for sr in (2, 0):
        ref = full if sr == 2 else ops.roi_align_fpn_nhwc(nh, boxes, lvl, (res, res), scales, 0)
        for word, live in _counts(n):
            bh = boxes.clone(); lh = lvl.clone()
            bh[live:] = float("nan"); lh[live:] = 1 << 20                               # a dead box and its level are not even looked at
            out = torch.full((n, Cc, res, res), SENTINEL, device="cuda")
            ops._adopt_stream()
            ops.ctx._check(ops.ctx.lib.vido_roi_align_fpn_nhwc_n(ops.ctx.h, fp, Hs, Ws, sc, Cc, _p(bh), _p(lh), n, res, res, sr, _p(out), _p(_word(word))))
            assert torch.equal(out[:live], ref[:live]) and bool((out[live:] == SENTINEL).all()), (sr, word)
    assert torch.equal(ops.roi_align_fpn_nhwc(nh, boxes, lvl, (res, res), scales, 2, _word(n)), full)


def test_deconv2x2_with_a_live_count(ops):
    """n = 5 maps of 14 x 14: 196 columns per image, so the 128-column tiles straddle the live / dead boundary at every count from 1 to 4."""
    from vido_slam_amd.nets.ops import pack_deconv2x2
    n, cin, cout, H, W = 5, 256, 256, 14, 14
    lib = ops.ctx.lib
    assert lib.vido_deconv2x2_supported(n, cin, cout, H, W)
    g = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn(n, cin, H, W, generator=g)).cuda()
    w = torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5; b = torch.randn(cout, generator=g).cuda()
    wp = pack_deconv2x2(w).cuda()

    def run(xin, word, slope=0.0):
        y = torch.full((n, cout, 2 * H, 2 * W), SENTINEL, device="cuda")
        ops._adopt_stream()
        ops.ctx._check(lib.vido_deconv2x2_bias_act_n(ops.ctx.h, _p(xin), _p(wp), _p(b), _p(y), n, cin, cout, H, W, C.c_float(slope), _p(word)))
        return y
    full = run(x, None)
    assert bool((full != SENTINEL).all())
    conv = torch.nn.ConvTranspose2d(cin, cout, 2, 2, 0); conv.weight.data = w; conv.bias.data = b.cpu(); conv = conv.cuda()
    assert torch.equal(ops.deconv2x2_conv(conv, x, 0.0), full)
    torch.cuda.synchronize(); assert ops.conv1x1_range_flag() == 0
    for word, live in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (n + 5, n), (-2, 0)):
        y = run(_hostile_(x.clone(), live), _word(word))
        torch.cuda.synchronize()
        assert ops.conv1x1_range_flag() == 0, (word, "a dead row was read")
        assert torch.equal(y[:live], full[:live]), word
        assert bool((y[live:] == SENTINEL).all()), word
    assert torch.equal(ops.deconv2x2_conv(conv, x, 0.0, _word(n)), full)


def test_mask_logit_select_with_a_live_count(ops):
    n, c, H, W, classes = 7, 48, 5, 9, 3
    g = torch.Generator().manual_seed(5)
    feat = torch.relu(torch.randn(n, c, H, W, generator=g)).cuda(); conv = torch.nn.Conv2d(c, classes, 1)
    conv.weight.data = torch.randn(classes, c, 1, 1, generator=g) / c ** 0.5; conv.bias.data = torch.randn(classes, generator=g); conv = conv.cuda()
    labels = torch.randint(0, classes, (n,), generator=g).cuda()
    full = ops.mask_logit_select(feat, conv, labels)
    assert bool((full > 0).all())                                                      # a sigmoid: never exactly 0, so the zeros below are the dead slots' own
    for word, live in _counts(n):
        got = ops.mask_logit_select(_hostile_(feat.clone(), live), conv, labels, _word(word))
        assert torch.equal(got[:live], full[:live]) and bool((got[live:] == 0).all()), word


def test_det_order_also_writes_the_count_as_int32(ops):
    g = torch.Generator().manual_seed(8)
    for cap, nd in ((100, 37), (100, 0), (20, 20)):
        scores = (torch.randint(0, 40, (cap,), generator=g).float() / 40).cuda(); labels = torch.randint(1, 81, (cap,), generator=g).cuda(); n_det = _word(nd)
        for conf in (0.8, -1.0, 2.0):
            o, l, n64 = ops.det_order(scores, labels, n_det, conf)
            o2, l2, n2, n32 = ops.det_order(scores, labels, n_det, conf, count32=True)
            assert torch.equal(o, o2) and torch.equal(l, l2) and int(n64) == int(n2) == int(n32[0]) and n32.dtype == torch.int32 and n64.dtype == torch.int64


# ---- graph level, on the tiny detector configuration -------------------------------------------------------------------------------------------------------------------
# The box head's GEMMs are not bit-reproducible from call to call (tests/test_e2e_gpu.py), and a score that moves by one ulp can move a slot across the confidence test.  So
# the two sides of every comparison below share ONE evaluation of the box head: _BoxHeadPin records what postprocess_fused returned and hands the same tensors to the next
# call.  `scale` (a device word) multiplies the scores — x 1.0 is exact, x 0.0 makes every slot fail the confidence test — so that a captured graph can be replayed on a
# frame without live slots.
class _BoxHeadPin:
    def __init__(self, box_head):
        self.fn = box_head.postprocess_fused; self.fixed = None; self.last = None; self.scale = torch.ones((), device="cuda")
        box_head.postprocess_fused = self

    def __call__(self, *a):
        if self.fixed is not None:
            return self.fixed
        b, s, l, n = self.fn(*a)
        self.last = (b, s * self.scale, l, n)
        return self.last

    def pin(self):
        self.fixed = tuple(t.clone() for t in self.last)


FEED = (96, 128)                                                                       # the fixture's image, fed as it is
OUT_HW = (120, 200)
CONF_SOME = float(np.median(G["det_scores"]))                                          # the fixture's 20 detections score 0.211 .. 0.233


@pytest.fixture(scope="module")
def tiny(ctx, ops):
    net = nets.fill_maskrcnn(nets.MaskRCNN(ops, TINY), int(G["seed"])).eval().cuda()
    return net, _BoxHeadPin(net.roi_heads.box)


def _reference(net, feats, logits, deltas, confidence, mode):
    """heads_static (default: every slot's mask, slot order) + label_image_torch on the slots the box head filled"""
    out = net.heads_static(feats, logits, deltas, FEED)
    assert "order" not in out
    n = min(int(out["n_det"]), out["boxes"].shape[0])
    H, W = OUT_HW
    boxes = out["boxes"] * out["boxes"].new_tensor([W / FEED[1], H / FEED[0], W / FEED[1], H / FEED[0]])
    img, labels = nets.label_image_torch(out["masks"][:n], boxes[:n], out["scores"][:n], out["labels"][:n], H, W, confidence, mode)
    return img, labels, n


@pytest.mark.parametrize("mode", ["class", "instance"])
def test_analyse_image_static_equals_the_full_mask_head(tiny, mode):
    net, pin = tiny
    image = torch.from_numpy(G["image"])[None].cuda()
    with torch.no_grad():
        feats, logits, deltas = net.trunk(image)
        for conf in (2.0, CONF_SOME, -1.0):
            pin.fixed = None; pin.scale.fill_(1.0)
            img, labels, n_live, n_det = nets.analyse_image_static(net, feats, logits, deltas, OUT_HW, feed=FEED, confidence=conf, label_mode=mode)
            assert pin.last[3].dtype == torch.int32                                   # the fused selection: the path that orders before the mask head
            pin.pin()
            ref_img, ref_labels, n = _reference(net, feats, logits, deltas, conf, mode)
            # the three cases are a condition on the inputs: none, some, all of the detections live
            k = len(ref_labels)
            assert n > 2 and (k == 0 if conf == 2.0 else k == n if conf == -1.0 else 0 < k < n), (conf, k, n)
            assert int(n_det) == n and int(n_live) == k
            assert torch.equal(labels[:k], ref_labels) and bool((labels[k:] == 0).all())
            assert torch.equal(img, ref_img), (conf, float((img != ref_img).float().mean()))
            # and the switch that restores the full mask head gives the same
            os.environ["VIDO_MASK_HEAD_ALL"] = "1"
            try:
                img_a, labels_a, n_live_a, _ = nets.analyse_image_static(net, feats, logits, deltas, OUT_HW, feed=FEED, confidence=conf, label_mode=mode)
            finally:
                del os.environ["VIDO_MASK_HEAD_ALL"]
            assert torch.equal(img_a, img) and torch.equal(labels_a, labels) and int(n_live_a) == k
        pin.fixed = None


def test_heads_static_with_a_confidence_gives_the_live_slots_their_masks(tiny):
    """slot for slot: the ordered call's mask of a live slot is the default call's mask of the same box, a dead slot's is 0"""
    net, pin = tiny
    image = torch.from_numpy(G["image"])[None].cuda()
    with torch.no_grad():
        feats, logits, deltas = net.trunk(image)
        pin.fixed = None; pin.scale.fill_(1.0)
        out = net.heads_static(feats, logits, deltas, FEED, None, CONF_SOME)
        pin.pin()
        ref = net.heads_static(feats, logits, deltas, FEED)
        pin.fixed = None
    k = int(out["n_live"])
    assert 0 < k < int(out["n_det"])
    assert torch.equal(out["masks"][:k], ref["masks"][out["order"][:k]]) and bool((out["masks"][k:] == 0).all())
    assert torch.equal(out["labels_ordered"][:k], ref["labels"][out["order"][:k]]) and bool((out["labels_ordered"][k:] == 0).all())


def test_captured_graph_replays_with_the_live_count_of_each_frame(tiny):
    """One capture of trunk + heads + label image; every replay reads its own frame's count.  Three images whose live counts differ, then a frame without live slots after
    one with some: no stale mask reaches the image."""
    from vido_slam_amd.nets.fuse import Graphed
    net, pin = tiny
    base = torch.from_numpy(G["image"])[None].cuda()
    images = [base, base.flip(-1).contiguous(), base.flip(-2).contiguous()]
    pin.fixed = None; pin.scale.fill_(1.0)

    def fn(image):
        feats, logits, deltas = net.trunk(image)
        img, labels, n_live, n_det = nets.analyse_image_static(net, feats, logits, deltas, OUT_HW, feed=FEED, confidence=CONF_SOME, label_mode="instance")
        return (img, labels, n_live, n_det) + tuple(feats) + tuple(logits) + tuple(deltas)
    with torch.no_grad():
        g = Graphed(fn, [base])
        nf = len(net.trunk(base)[0]); nl = (len(g.static_out) - 4 - nf) // 2
        lives = []
        for image, scale in list(zip(images, (1.0, 1.0, 1.0))) + [(base, 0.0)]:
            pin.fixed = None; pin.scale.fill_(scale)
            out = [t.clone() for t in g(image)]
            img, labels, n_live, n_det = out[:4]
            feats, logits, deltas = out[4:4 + nf], out[4 + nf:4 + nf + nl], out[4 + nf + nl:]
            pin.pin()                                                                  # the replay's own box-head results (the capture's static tensors)
            e_img, e_labels, e_live, e_det = nets.analyse_image_static(net, feats, logits, deltas, OUT_HW, feed=FEED, confidence=CONF_SOME, label_mode="instance")
            r_img, r_labels, n = _reference(net, feats, logits, deltas, CONF_SOME, "instance")
            pin.fixed = None
            k = int(n_live); lives.append(k)
            print("replay: scale %.1f live %d of %d" % (scale, k, int(n_det)))
            assert int(e_live) == k == len(r_labels) and int(e_det) == int(n_det) == n
            assert torch.equal(labels, e_labels) and torch.equal(img, e_img)
            assert torch.equal(labels[:k], r_labels) and torch.equal(img, r_img)
            if scale == 0.0:
                assert k == 0 and int(img.max()) == 0
        pin.scale.fill_(1.0)
    assert len(set(lives[:3])) == 3 and lives[2] > 0, lives      # a condition on the inputs: three different counts, the one before the empty frame not 0
