"""The four split-fp16 entry points — HipOps.conv1x1_bias_act (pack layout 3, csrc/conv1x1.hip k_conv1x1_b3<NP 2>), conv3x3_h_bias_act (csrc/conv3x3h.hip), fc_h
(csrc/fch.hip) and deconv2x2_conv (csrc/conv1x1.hip, RES 3) — against float64 on HOSTILE inputs: the edges the kernels document for themselves (the 2.5e-4 .. 65504
full-precision band of the activations and the absolute-error floor below it, per-row power-of-two weight scales over rows with a large dynamic range, the zero-padded
input channels of a ragged 3x3 layer, the range flag).  tests/test_maskrcnn_gpu.py checks the same kernels on Gaussian data.

The elementwise bound.  For every output y (after bias, residual and activation) and its float64 value y64, with the sums over that output's contraction (K products) in
float64:

    |y - y64| <= 2^-23 max(8, sqrt K) sum|w x| + 2^-34 sum|w| + 2^-23 (|bias| + |residual|)

  * 2^-23 max(8, sqrt K) sum|w x| — 2^-20 sum|w x| up to K = 64: the fp32 FMA-chain envelope (an exact fmaf chain: 0.75 - 3.5e-7 sum|w x| on uniform operands at K <= 1024,
    about 2^-22 .. 2^-21); the split-fp16 form represents each operand to 2^-22 relative (two roundings to 11 bits) and rounds once per 16 products.  Past K = 64 the term grows
    as sqrt K: a chain of K roundings whose partial sums sit at the scale of sum|w x| (a few products dominate a heavy-tailed row, case (b)) random-walks to about
    sqrt(K) 2^-24 sum|w x| at the worst of millions of outputs — MEASURED on the MI355X with the fixed 2^-20: the fp32 forms reach 1.9x it at K = 1024 (the fp32
    matrix instruction), 1.2x at 256 (the library's transposed convolution), 4.0x at 12544 (the library GEMM), the library's default 3x3 algorithm 9.8x at 2304; the split-fp16
    kernels 0.91x / 0.81x / 0.98x / 0.96x.  The term is 2x that random walk, and never below the K-free 2^-20.
  * 2^-34 sum|w|: an activation below fp16's normal range (|x| < 2^-14; h subnormal) keeps an ABSOLUTE error <= 2^-36 (l' = rne16(2^11 (x - h)) is itself subnormal, spacing
    2^-24, rounding <= 2^-25, divided by 2^11); times |w| per product.  The term is 4x that floor.  Weights have no such floor: each row is scaled by a power of two that
    puts its largest |w| into [2^14, 2^15), and what is lost below 2^-26 of the row's maximum is covered by the first term.
  * 2^-23 (|bias| + |residual|): the epilogue's fp32 additions (and the activation's product), one rounding each.
  The leaky ReLU (slope in [0, 1]) is 1-Lipschitz, so the bound on the pre-activation carries over.

The bound checks itself: on the same inputs the fp32 forms pass it too — the fp32 matrix instruction (conv1x1_set_arith(1)) for the 1x1, the library's fp32 linear and
conv_transpose2d, and for the 3x3 the library's direct (im2col + GEMM) form: the algorithm MIOpen picks by default (a transform-based one) amplifies rounding
beyond any chain envelope (above).  For cases (a) and (b) the rule of tests/test_maskrcnn_gpu.py holds as well: max and rms of |y - y64| / bound <= 1.5x the fp32 form's.

Measured on the MI355X (the table `pytest -s` prints: profiles/r7/split_fp16_errors.txt): the split-fp16 kernels reach at most 0.43 of the bound over all cases and
shapes, the fp32 forms 0.62; in cases (a) and (b) the split form's max / rms is at most 1.10x / 1.28x the fp32 form's (the small transposed convolution), 0.1 - 0.7x
elsewhere.  Broken builds this file catches: the 1x1 kernel without its w_l x_h product, the 3x3 kernel with the h plane of the weights only, fc_h without the inverse
row scale (each fails every bound case of its kernel); before the fixes that came with it, a NaN activation left the flag down and a ragged 3x3 layer passed the next
image's infinities and NaNs into this image's outputs."""
import math
import pytest
import torch

pytestmark = pytest.mark.gpu
F = torch.nn.functional
FLOOR, EPI = 2.0 ** -34, 2.0 ** -23
KINDS = ("c1", "c3", "fc", "dc")
# (name, shape): c1 (cin, cout, H, W) / c3 (N, cin, cout, H, W) / fc (rows, k, outs) / dc (N, cin, cout, H, W)
SHAPES = {"c1": (("detector", (1024, 256, 50, 68)), ("ragged", (160, 384, 13, 21))),          # FPN lateral of P4 / 273 positions (not a multiple of the 128-wide tile)
          "c3": (("detector", (1, 256, 256, 50, 68)), ("ragged", (2, 49, 128, 30, 40))),      # FPN output / RPN head at P4 / 49 input channels (last chunk padded) over a batch
          "fc": (("detector", (1000, 12544, 1024)), ("ragged", (333, 2048, 256))),            # the box head's fc6 / ragged rows
          "dc": (("detector", (100, 256, 256, 14, 14)), ("ragged", (3, 64, 128, 6, 10)))}      # the mask head's transposed convolution / a small batch of odd maps


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ops(ctx):
    from vido_slam_amd.nets.ops import HipOps
    o = HipOps(ctx)
    assert o.conv1x1_set_arith(0) == 0, "these tests need the default arithmetic (split-fp16) at the start"
    o.conv1x1_range_flag(reset=True)
    return o


def dims(kind, shape):
    """(x shape, w shape, cout, K): K = the contraction length of one output"""
    if kind == "c1":
        cin, cout, H, W = shape; return (1, cin, H, W), (cout, cin, 1, 1), cout, cin
    if kind == "c3":
        n, cin, cout, H, W = shape; return (n, cin, H, W), (cout, cin, 3, 3), cout, 9 * cin
    if kind == "fc":
        rows, k, outs = shape; return (rows, k), (outs, k), outs, k
    n, cin, cout, H, W = shape; return (n, cin, H, W), (cin, cout, 2, 2), cout, cin


def to_rows(kind, w):
    """the weight as the GEMM's [rows, K] matrix (a row = what one power-of-two scale covers)"""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]) if kind == "dc" else w.reshape(w.shape[0], -1)


def from_rows(kind, m, wshape):
    if kind == "dc":
        cin, cout = wshape[0], wshape[1]
        return m.reshape(2, 2, cout, cin).permute(3, 2, 0, 1).contiguous()
    return m.reshape(wshape).contiguous()


def contract(kind, x, w):
    """the linear part in float64 on the host (float64 convolutions have no library kernel on the device)"""
    x, w = x.double(), w.double()
    if kind == "c1":
        return F.conv2d(x, w)
    if kind == "c3":
        return F.conv2d(x, w, padding=1)
    if kind == "fc":
        return F.linear(x.cuda(), w.cuda()).cpu()              # (float64 GEMM on the device)
    return F.conv_transpose2d(x, w, stride=2)


def bcast(kind, v):
    return v.double()[None, :] if kind == "fc" else v.double()[None, :, None, None]


def reference(kind, x, w, b, r, slope, K):
    """(y64, bound): float64 output after the activation and the elementwise bound of the module docstring (K: the products per output)"""
    pre = contract(kind, x, w)
    s1 = contract(kind, x.abs(), w.abs())
    s2 = contract(kind, torch.ones_like(x), w.abs())
    s3 = torch.zeros_like(pre)
    if b is not None:
        pre = pre + bcast(kind, b); s3 = s3 + bcast(kind, b).abs()
    if r is not None:
        pre = pre + r.double(); s3 = s3 + r.double().abs()
    return F.leaky_relu(pre, slope), 2.0 ** -23 * max(8.0, math.sqrt(K)) * s1 + FLOOR * s2 + EPI * s3


def run_split(kind, ops, x, w, b, r, slope):
    from vido_slam_amd.nets.ops import pack_conv1x1, pack_conv3x3_h
    bc = b.cuda() if b is not None else None
    if kind == "c1":
        cin, cout, hw = x.shape[1], w.shape[0], x.shape[2] * x.shape[3]
        assert ops.conv1x1_layout(cin, cout, hw) == 3
        return ops.conv1x1_bias_act(x.cuda(), pack_conv1x1(w, 3).cuda(), bc, r.cuda() if r is not None else None, slope).cpu()
    if kind == "c3":
        assert ops.ctx.lib.vido_conv3x3_h_supported(*x.shape[:2], w.shape[0], *x.shape[2:])
        return ops.conv3x3_h_bias_act(x.cuda(), pack_conv3x3_h(w).cuda(), bc, int(w.shape[0]), slope).cpu()
    if kind == "fc":
        y = ops.fc_h(x.cuda(), pack_conv1x1(w.reshape(w.shape[0], w.shape[1], 1, 1), 3).cuda(), bc, int(w.shape[0]), slope)
        assert y is not None
        return y.cpu()
    conv = torch.nn.ConvTranspose2d(w.shape[0], w.shape[1], 2, 2, 0, bias=b is not None)
    conv.weight.data = w.clone()
    if b is not None:
        conv.bias.data = b.clone()
    y = ops.deconv2x2_conv(conv.cuda(), x.cuda(), slope)
    assert y is not None
    return y.cpu()


def run_fp32(kind, ops, x, w, b, r, slope):
    """the fp32 form of the same operation on the same inputs"""
    from vido_slam_amd.nets.ops import pack_conv1x1
    bc = b.cuda() if b is not None else None
    if kind == "c1":
        cin, cout, hw = x.shape[1], w.shape[0], x.shape[2] * x.shape[3]
        prev = ops.conv1x1_set_arith(1)
        try:                                                      # (packed AFTER the switch: a packed weight carries the layout of the arithmetic it was packed for)
            lay = ops.conv1x1_layout(cin, cout, hw)
            assert lay in (0, 1)
            return ops.conv1x1_bias_act(x.cuda(), pack_conv1x1(w, lay).cuda(), bc, r.cuda() if r is not None else None, slope).cpu()
        finally:
            ops.conv1x1_set_arith(prev)
    if kind == "c3":
        with torch.backends.cudnn.flags(enabled=False):           # (the direct form: MIOpen's default Winograd is no fmaf chain — module docstring)
            return F.leaky_relu(F.conv2d(x.cuda(), w.cuda(), bc, padding=1), slope).cpu()
    if kind == "fc":
        return F.leaky_relu(F.linear(x.cuda(), w.cuda(), bc), slope).cpu()
    return F.leaky_relu(F.conv_transpose2d(x.cuda(), w.cuda(), bc, stride=2), slope).cpu()


def measure(y, y64, bound):
    q = (y.double() - y64).abs() / bound.clamp_min(1e-300)
    return float(q.max()), float(q.pow(2).mean().sqrt())


def make_case(kind, shape, case, seed):
    """inputs of case (a) / (b) / (c): (x, w, bias, residual, slope)"""
    g = torch.Generator().manual_seed(seed)
    xs, ws, cout, K = dims(kind, shape)
    cin = xs[1]
    ch_view = (1, cin) if kind == "fc" else (1, cin, 1, 1)
    b = r = None
    if case == "a":      # post-ReLU activations (about half zeros), per-input-channel scales 10^U(-2, 2); ordinary weights, bias (+ a residual for the 1x1)
        x = torch.relu(torch.randn(xs, generator=g)) * torch.pow(10.0, torch.rand(ch_view, generator=g) * 4 - 2)
        w = torch.randn(ws, generator=g) / math.sqrt(K)
        b = torch.randn(cout, generator=g)
        if kind == "c1":
            r = torch.randn(1, cout, xs[2], xs[3], generator=g)
        slope = 0.0
    elif case == "b":    # heavy-tailed weights per element; an all-zero row (a folded batch norm with gamma = 0), a row with one non-zero weight, weights at 2^-30 of their row's maximum
        x = torch.relu(torch.randn(xs, generator=g))
        m = to_rows(kind, torch.randn(ws, generator=g) * torch.exp(2 * torch.randn(ws, generator=g))).clone()
        m[0] = 0.0
        keep = m[1, 3].item(); m[1] = 0.0; m[1, 3] = keep if keep != 0 else 1.0
        for row in (2, 5, m.shape[0] - 1):
            mx = float(m[row].abs().max())
            m[row, :7] = mx * 2.0 ** -30 * torch.sign(torch.randn(7, generator=g))
        w = from_rows(kind, m, ws)
        b = torch.randn(cout, generator=g) * 0.1
        slope = 0.1
    else:                # activations log-uniform in [1e-6, 1e-4] with random signs: below fp16's normal range (h subnormal); no bias (it would hide the floor)
        x = torch.exp(torch.rand(xs, generator=g) * (math.log(1e-4) - math.log(1e-6)) + math.log(1e-6)) * torch.sign(torch.randn(xs, generator=g))
        w = torch.randn(ws, generator=g) / math.sqrt(K)
        slope = 1.0
    return x, w, b, r, slope


@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("kind", KINDS)
def test_split_fp16_within_the_elementwise_bound(vido, ops, kind, case):
    """Cases (a) post-ReLU activations with per-channel scales over 10^4, (b) heavy-tailed weights with a zero row, a one-weight row and weights at 2^-30 of their row's
    maximum, (c) activations below fp16's normal range (if fp16 subnormals were flushed anywhere on the path, this case fails: h = 0 loses up to 6e-5 per activation,
    2^18 times the floor) — each at a detector shape and a ragged one: every output within the bound (module docstring), the fp32 form within it too, and for (a), (b) the
    split form's max and rms of |y - y64| / bound at most 1.5x the fp32 form's.  The range flag stays down."""
    fails = []
    for si, (name, shape) in enumerate(SHAPES[kind]):
        x, w, b, r, slope = make_case(kind, shape, case, 1000 * KINDS.index(kind) + 10 * si + ord(case))
        y64, bound = reference(kind, x, w, b, r, slope, dims(kind, shape)[3])
        ys = run_split(kind, ops, x, w, b, r, slope)
        yf = run_fp32(kind, ops, x, w, b, r, slope)
        assert ys.shape == yf.shape == y64.shape
        ms, rs = measure(ys, y64, bound)
        mf, rf = measure(yf, y64, bound)
        print("split-fp16 %s case %s, %s %s: max %.3f rms %.4f of the bound | fp32 form: max %.3f rms %.4f | ratio max %.2f rms %.2f"
              % (kind, case, name, shape, ms, rs, mf, rf, ms / max(mf, 1e-30), rs / max(rf, 1e-30)))
        if not (ms <= 1.0):
            fails.append((name, "split-fp16 outside the bound", ms))
        if not (mf <= 1.0):
            fails.append((name, "fp32 form outside the bound (the bound is wrong)", mf))
        if case in ("a", "b") and not (ms <= 1.5 * mf and rs <= 1.5 * rf):
            fails.append((name, "split-fp16 noisier than 1.5x the fp32 form", ms, mf, rs, rf))
    torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0
    assert not fails, fails


def _ragged(kind):
    return SHAPES[kind][1][1]


@pytest.mark.parametrize("kind", KINDS)
def test_split_fp16_range_edges_and_the_flag(vido, ops, kind):
    """(d) the largest activation 65000: flag down and every output within the bound; one element of exactly 65504, -70000, +inf or NaN: the flag is raised, and the read
    resets it (the second read gives 0).  A NaN used to slip past the flag: fmaxf returns the operand that is not a NaN."""
    shape = _ragged(kind)
    x, w, b, r, slope = make_case(kind, shape, "a", 77 + KINDS.index(kind))
    x = torch.relu(torch.randn(x.shape, generator=torch.Generator().manual_seed(3)))
    at = (5, 17) if kind == "fc" else (0, 3, 2, 4)
    ops.conv1x1_range_flag(reset=True)
    xe = x.clone(); xe[at] = 65000.0
    y64, bound = reference(kind, xe, w, b, r, slope, dims(kind, shape)[3])
    ys = run_split(kind, ops, xe, w, b, r, slope); torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0, "65000 is inside fp16's range"
    ms, _ = measure(ys, y64, bound)
    assert ms <= 1.0, ms
    for v in (65504.0, -70000.0, math.inf, math.nan):
        xe = x.clone(); xe[at] = v
        run_split(kind, ops, xe, w, b, r, slope); torch.cuda.synchronize()
        assert ops.conv1x1_range_flag(reset=True) == 1, (kind, v)
        assert ops.conv1x1_range_flag(reset=True) == 0, (kind, v)


def test_split_fp16_range_flags_are_per_context(vido, ops):
    """(e) an overflow on one Context raises that context's flag and leaves another context's at 0 (both ways, through two different kernels)."""
    from vido_slam_amd.nets.ops import HipOps
    ctx2 = vido.Context()
    try:
        ops2 = HipOps(ctx2)
        ops.conv1x1_range_flag(reset=True); ops2.conv1x1_range_flag(reset=True)
        for first, second, kind in ((ops, ops2, "c1"), (ops2, ops, "c3")):
            x, w, b, r, slope = make_case(kind, _ragged(kind), "a", 5)
            x[(0, 1, 2, 3)] = 70000.0
            run_split(kind, first, x, w, b, r, slope); torch.cuda.synchronize()
            assert second.conv1x1_range_flag(reset=True) == 0, kind
            assert first.conv1x1_range_flag(reset=True) == 1, kind
    finally:
        ctx2.close()


@pytest.mark.parametrize("cin", [49, 131])
@pytest.mark.parametrize("poison", [1e5, math.nan])
def test_conv3x3_h_padded_channels_do_not_read_the_next_image(vido, ops, cin, poison):
    """(f) k_conv3x3_h with cin % 16 != 0 pads the last chunk with zero weights; its window covers the NEXT image's first channels.  Image 1 holds 1e5 (an fp16 infinity) or
    a NaN in all of channel 0: image 0's outputs stay finite and within the bound (inf x 0 = NaN would spread into every one of them).  The flag may be raised — image 1
    overflowed."""
    g = torch.Generator().manual_seed(cin)
    x = torch.relu(torch.randn(2, cin, 20, 36, generator=g)); w = torch.randn(128, cin, 3, 3, generator=g) / math.sqrt(9 * cin); b = torch.randn(128, generator=g)
    x[1, 0] = poison
    y = run_split("c3", ops, x, w, b, None, 0.1)
    torch.cuda.synchronize(); ops.conv1x1_range_flag(reset=True)
    y64, bound = reference("c3", x[:1], w, b, None, 0.1, 9 * cin)
    assert bool(torch.isfinite(y[0]).all()), "image 0 contaminated by image 1's padded channels"
    ms, _ = measure(y[:1], y64, bound)
    assert ms <= 1.0, ms
