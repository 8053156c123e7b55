"""The mask head's counted launches choose their form from the live count ON THE DEVICE (csrc/conv3x3h.hip k_conv3x3_h_live; csrc/nets.hip: the mask pooler's bins split
over workgroups, the logit kernel's batched loads, the label image's walk that stops at the count).  Every form computes every element in the same order from the same
operands, so every comparison here is torch.equal against the uncounted call, which launches what it always launched.

Dead rows of the inputs hold NaN, infinity and 70000 (what a stale buffer may hold): they must stay unread — the split-fp16 range flag stays 0 — and the dead rows of the
outputs keep a sentinel.  Nothing here provokes a fault: the hostile values are data in rows that must not be read."""
import ctypes as C
import numpy as np
import pytest
import torch
from vido_slam_amd import nets

pytestmark = pytest.mark.gpu
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


def _clamp(word, n):
    return min(max(word, 0), n)


def _fine_max(ops, n, cout, h, w):
    """T: the largest count word in [0, n] that the rule sends to the fine form (read from the library, not restated here)"""
    fine = [ops.conv3x3_h_live_form(n, cout, h, w, k)[0] for k in range(n + 1)]
    assert fine[0], "a count of 0 takes the fine form"
    T = max(k for k in range(n + 1) if fine[k])
    assert all(fine[:T + 1]) and not any(fine[T + 1:]), "one threshold"
    return T


def _conv3x3_n(ops, x, wp, b, y, cout, slope, word):
    n, cin, h, w = x.shape
    ops._adopt_stream()
    ops.ctx._check(ops.ctx.lib.vido_conv3x3_h_bias_act_n(ops.ctx.h, _p(x), _p(wp), _p(b), _p(y), n, cin, cout, h, w, C.c_float(slope), _p(word)))


def _conv_case(n, cin, cout, H, W):
    from vido_slam_amd.nets.ops import pack_conv3x3_h
    g = torch.Generator().manual_seed(1000 * n + cin + H)
    x = torch.randn(n, cin, H, W, generator=g).cuda()
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5); b = torch.randn(cout, generator=g).cuda()
    return x, pack_conv3x3_h(w).cuda(), b


# (n, cin, cout, h, w, the host picks the 16-row form for n images).  14 x 14 with one and two K chunks (cin 16 / 32: the weight ring wraps, the window buffer toggles) and
# 128 output channels; the mask head's real channel counts on a batch the host runs in the 8-row form; 9 x 9 (a block overhanging the edge) and 17 x 20 (more than one block
# per image in both directions, overhanging) with a fine form serving 256 channels
CONV_CASES = [(100, 16, 256, 14, 14, True), (100, 32, 256, 14, 14, True), (200, 16, 128, 14, 14, True), (24, 256, 256, 14, 14, False), (100, 16, 256, 9, 9, True), (100, 16, 256, 17, 20, True)]


@pytest.mark.parametrize("n,cin,cout,H,W,rows16", CONV_CASES)
def test_counted_conv3x3_equals_the_uncounted_call_in_both_forms(ops, n, cin, cout, H, W, rows16):
    lib = ops.ctx.lib
    assert not lib.vido_mask_head_coarse(), "VIDO_MASK_HEAD_COARSE is set: the fine form is off"
    coarse_wgs = n * ((H + 15) // 16) * ((W + 15) // 16) * (cout // 128)
    assert (lib.vido_conv3x3_h_workgroups(n, cout, H, W) == coarse_wgs) == rows16                   # the uncounted launch: 16-row blocks, or 8-row ones
    T = _fine_max(ops, n, cout, H, W)
    assert T >= 1
    fT, fT1 = ops.conv3x3_h_live_form(n, cout, H, W, T), ops.conv3x3_h_live_form(n, cout, H, W, T + 1)
    assert fT[0] and fT[1] < 128 and cout // fT[1] >= 2                                              # a fine form: several channel tiles where the coarse one has cout / 128
    if T < n:                                                                                        # the rule switches inside the batch: both bodies of the kernel run below
        assert not fT1[0] and fT1[1:] == (128, 16 if rows16 else 8) and fT1[1:] != fT[1:]
    else:                                                                                            # every count of this batch is fine; the coarse form is the uncounted call's
        assert (128, 16 if rows16 else 8) != fT[1:]
    x, wp, b = _conv_case(n, cin, cout, H, W)
    full = ops.conv3x3_h_bias_act(x, wp, b, cout, 0.0)
    torch.cuda.synchronize(); assert ops.conv1x1_range_flag() == 0
    for word in (-2, 0, 1, T, T + 1, n, n + 5):
        live = _clamp(word, n)
        xh = _hostile_(x.clone(), live)
        y = torch.full((n, cout, H, W), SENTINEL, device="cuda")
        _conv3x3_n(ops, xh, wp, b, y, cout, 0.0, _word(word))
        torch.cuda.synchronize()
        assert ops.conv1x1_range_flag() == 0, (word, "a dead row was read")
        assert torch.equal(y[:live], full[:live]), word
        assert bool((y[live:] == SENTINEL).all()), word
    y = torch.full((n, cout, H, W), SENTINEL, device="cuda")                                          # a NULL count: the uncounted launch
    _conv3x3_n(ops, x, wp, b, y, cout, 0.0, None)
    assert torch.equal(y, full)


def test_forced_forms_agree_bit_for_bit(ops):
    """the measurement entry point (tools/prof_mask_head_live.py forms): every form of the kernel on the same input"""
    n, cin, cout, H, W = 3, 32, 256, 17, 20
    x, wp, b = _conv_case(n, cin, cout, H, W)
    full = ops.conv3x3_h_bias_act(x, wp, b, cout, 0.0)
    for rpw, cg in ((4, 1), (2, 2), (2, 1), (1, 2), (1, 1)):
        y = torch.full((n, cout, H, W), SENTINEL, device="cuda")
        ops._adopt_stream()
        ops.ctx._check(ops.ctx.lib.vido_conv3x3_h_bias_act_form(ops.ctx.h, _p(x), _p(wp), _p(b), _p(y), n, cin, cout, H, W, C.c_float(0.0), rpw, cg))
        assert torch.equal(y, full), (rpw, cg)


def _kernel_nodes(graph):
    """kernel nodes of a captured graph (torch keeps the graph: CUDAGraph(keep_graph=True))"""
    hip = C.CDLL("libamdhip64.so")
    g = C.c_void_p(graph.raw_cuda_graph())
    cnt = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(cnt)) == 0
    nodes = (C.c_void_p * cnt.value)()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(cnt)) == 0
    kinds = []
    for nd in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nd), C.byref(t)) == 0
        kinds.append(t.value)
    return sum(1 for t in kinds if t == 0), len(kinds)                                                # hipGraphNodeTypeKernel = 0


def test_one_captured_launch_follows_the_count_of_each_replay(ops):
    n, cin, cout, H, W = 100, 16, 256, 14, 14
    T = _fine_max(ops, n, cout, H, W)
    assert T + 3 < n
    x, wp, b = _conv_case(n, cin, cout, H, W)
    full = ops.conv3x3_h_bias_act(x, wp, b, cout, 0.0)
    word = _word(n); y = torch.empty((n, cout, H, W), device="cuda")
    _conv3x3_n(ops, x, wp, b, y, cout, 0.0, word)                                                     # warm-up outside the capture (the LDS attributes)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    s = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        _conv3x3_n(ops, x, wp, b, y, cout, 0.0, word)
    assert _kernel_nodes(g)[0] == 1                                                                   # one layer, one kernel node (and nothing else)
    g.instantiate()
    for v in (2, T + 3, 0, n, 3):
        word.fill_(v); y.fill_(SENTINEL)
        g.replay(); torch.cuda.synchronize()
        assert torch.equal(y[:v], full[:v]) and bool((y[v:] == SENTINEL).all()), v
    assert ops.conv1x1_range_flag() == 0


# ---- the mask pooler ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [14, 5])
def test_mask_pooler_split_over_workgroups(ops, oracle, res):
    """14 x 14 = 196 bins and 5 x 5 = 25: both leave a ragged last segment of bins; 80 channels: a full 64-channel group and a ragged one; 9 boxes over the 4 levels,
    partly outside the maps.  The counted call splits a roi's bins over workgroups, the uncounted one does not."""
    n, Cc = 9, 80
    rng = np.random.RandomState(3)
    feats = [torch.randn(1, Cc, 24 >> l, 32 >> l, device="cuda") for l in range(4)]
    nh = [ops.to_nhwc(f) for f in feats]
    scales = (0.25, 0.125, 0.0625, 0.03125)
    xy = rng.uniform(-10, 90, (n, 2)); wh = rng.uniform(2, 70, (n, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).cuda()
    lvl = torch.from_numpy((np.arange(n) % 4).astype(np.int32)).cuda()
    full = ops.roi_align_fpn_nhwc(nh, boxes, lvl, (res, res), scales, 2)
    # the reference of the existing ROI-Align tests: the oracle, level by level
    rois = np.concatenate([np.zeros((n, 1), np.float32), boxes.cpu().numpy()], 1); lv = lvl.cpu().numpy(); got = full.cpu().numpy()
    for l in range(4):
        idx = np.nonzero(lv == l)[0]
        assert np.array_equal(got[idx], oracle.roi_align(feats[l].cpu().numpy(), rois[idx], scales[l], res, res, 2)), l
    fp = (C.c_void_p * 4)(*[f.data_ptr() for f in nh]); Hs = (C.c_int * 4)(*[f.shape[1] for f in nh]); Ws = (C.c_int * 4)(*[f.shape[2] for f in nh]); sc = (C.c_float * 4)(*scales)
    T = 4                                                                                            # (no threshold in this kernel: the counts around a middle one)
    for word in (-2, 0, 1, T, T + 1, n, n + 5):
        live = _clamp(word, n)
        bh = boxes.clone(); lh = lvl.clone()
        bh[live:] = float("nan"); lh[live:] = 1 << 20                                                 # a dead box and its level are not even looked at
        out = torch.full((n, Cc, res, res), SENTINEL, device="cuda")
        ops._adopt_stream()
        ops.ctx._check(ops.ctx.lib.vido_roi_align_fpn_nhwc_n(ops.ctx.h, fp, Hs, Ws, sc, Cc, _p(bh), _p(lh), n, res, res, 2, _p(out), _p(_word(word))))
        assert torch.equal(out[:live], full[:live]) and bool((out[live:] == SENTINEL).all()), word


# ---- the logit kernel ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [256, 20, 7, 3])
@pytest.mark.parametrize("hw", [(28, 28), (5, 10)])
def test_logit_select_with_batched_loads(ops, c, hw):
    """c = 256: whole batches of loads; 20, 7, 3: the tails behind them (groups of four, single channels).  The counted call (batched loads) against the uncounted one (the
    loop as it was): the same addends into the same four float64 sums, so the same bits; and both against sigmoid of a float64 restatement within 4 ulps of fp32 at 1.0
    (the kernel rounds the float64 sum to fp32 once and takes expf of it)."""
    n, classes = 6, 5
    H, W = hw
    g = torch.Generator().manual_seed(c + H)
    feat = torch.relu(torch.randn(n, c, H, W, generator=g)).cuda(); conv = torch.nn.Conv2d(c, classes, 1)
    conv.weight.data = torch.randn(classes, c, 1, 1, generator=g) / c ** 0.5; conv.bias.data = torch.randn(classes, generator=g); conv = conv.cuda()
    labels = torch.randint(0, classes, (n,), generator=g).cuda()
    full = ops.mask_logit_select(feat, conv, labels)
    wsel = conv.weight.data.double()[labels, :, 0, 0]                                                 # [n, c]
    ref = torch.sigmoid((wsel[:, :, None, None] * feat.double()).sum(1) + conv.bias.data.double()[labels][:, None, None])
    err = float((full.reshape(n, H, W).double() - ref).abs().max())
    print("logit select c %d hw %d: max |kernel - float64 sigmoid| %.3g" % (c, H * W, err))
    assert err <= 4 * 2.0 ** -23, err                                                                 # 4.8e-7
    for word in (-2, 0, 1, 3, 4, n, n + 5):
        live = _clamp(word, n)
        got = ops.mask_logit_select(_hostile_(feat.clone(), live), conv, labels, _word(word))
        assert torch.equal(got[:live], full[:live]) and bool((got[live:] == 0).all()), word


# ---- the label image ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("live", [0, 3, 20])
def test_label_image_walk_stops_at_the_live_count(ops, live):
    """20 slots, the first `live` of them with a class and a mask, the others as the static head leaves them: label 0, zero masks, boxes of their own"""
    nd, Hh, Ww = 20, 120, 200
    rng = np.random.RandomState(7 + live)
    masks = torch.rand(nd, 1, 28, 28, device="cuda"); masks[live:] = 0
    xy = rng.uniform(-20, 150, (nd, 2)); wh = rng.uniform(3, 90, (nd, 2))
    bx = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).cuda()
    lab = rng.randint(1, 81, nd).astype(np.int64); lab[live:] = 0
    labels = torch.from_numpy(lab).cuda()
    full = ops.mask_label_image(masks, bx, labels, Hh, Ww)
    assert (int(full.max()) > 0) == (live > 0)
    for word in (live, nd, nd + 5):                                                                   # the count, and counts past it (the walk may go on over label-0 slots)
        assert torch.equal(ops.mask_label_image(masks, bx, labels, Hh, Ww, n_live=_word(word)), full), word
