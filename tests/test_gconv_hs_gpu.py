"""The split-fp16 grouped 3x3 kernel for 8 / 16 channels per group (csrc/gconvhs.hip: HipOps.gconv3x3_hs_bias_act, dispatched by HipOps.gconv3x3_conv) against
F.conv2d(..., groups=G) in float64 on the device, with the fp32 grouped kernel (HipOps.gconv3x3_bias_act, csrc/gconv.hip) on the same input as the yardstick.  Case generators,
reference and bound are those of tests/test_gconv_h_gpu.py (copied).

The hard condition on every case with a float64 reference is the elementwise bound of tests/test_split_fp16_gpu.py (its docstring derives the three terms), K = 9 x channels per
group:

    |y - y64| <= 2^-23 max(8, sqrt K) sum|w x| + 2^-34 sum|w| + 2^-23 |bias|

Inputs: (gauss) Gaussian post-ReLU activations, (x300) the same times 300, (sparse) nine tenths zeros with per-channel scales 10^U(-2, 2), (wtail) heavy-tailed per-output-
channel weight scales with an all-zero channel and a one-weight channel, (tiny) activations log-uniform in [1e-6, 1e-4] with random signs, no bias, no ReLU.  On (gauss) and
(x300) also: max and rms of |y - y64| / bound at most 1.5x the fp32 kernel's.

Shapes (groups x channels per group @ H x W): 2 x 8 @ 3 x 4 (smaller than a tile, both halo rows outside), 3 x 8 @ 17 x 20 (odd group count, ragged last tile, tiles across
row ends, two rounds), 2 x 8 @ 7 x 9 and 2 x 16 @ 9 x 12 (W no multiple of 4), 3 x 8 @ 3 x 140 (a row longer than a round: three rounds through the ring), 3 x 16 @ 5 x 33;
4 x 8 @ 40 x 272 and 4 x 16 @ 30 x 136 (full row width, several chunks per group, chunk boundaries mid-row); and the detector's 32 x 8 @ 200 x 272 and 32 x 16 @ 100 x 136
without a float64 reference: same bits run to run and from a captured graph, and the rows of a crop of the input (top rows; a slab in the middle with one halo row each side)
equal the full run's bit for bit — the order in which an output is summed does not depend on how the launch is cut into items and rounds."""
import ctypes as C
import math
import pytest
import torch

pytestmark = pytest.mark.gpu
F = torch.nn.functional
SMALL = ((2, 8, 3, 4), (3, 8, 17, 20), (2, 8, 7, 9), (2, 16, 9, 12), (3, 8, 3, 140), (3, 16, 5, 33))
WIDE = ((4, 8, 40, 272), (4, 16, 30, 136))
WORKLOAD = ((32, 8, 200, 272), (32, 16, 100, 136), (32, 8, 272, 200), (32, 16, 136, 100))      # (the last two: the maps the detector graph of bench.py launches, rows x columns)
CASES = ("gauss", "x300", "sparse", "wtail", "tiny")


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


def make_case(shape, case, seed):
    """-> (x, w, bias or None, slope) on the device"""
    G, cpg, H, W = shape
    g = torch.Generator().manual_seed(seed)
    Cn, K = G * cpg, 9 * cpg
    x = torch.relu(torch.randn(1, Cn, H, W, generator=g))
    w = torch.randn(Cn, cpg, 3, 3, generator=g) / math.sqrt(K)
    b = torch.randn(Cn, generator=g)
    slope = 0.0
    if case == "x300":
        x = x * 300.0
    elif case == "sparse":
        x = x * (torch.rand(x.shape, generator=g) < 0.1) * torch.pow(10.0, torch.rand(1, Cn, 1, 1, generator=g) * 4 - 2)
    elif case == "wtail":
        w = w * torch.exp(2 * torch.randn(Cn, 1, 1, 1, generator=g))
        w[0] = 0.0
        keep = float(w[1, 3, 1, 1]); w[1] = 0.0; w[1, 3, 1, 1] = keep if keep != 0 else 1.0
        b = b * 0.1
    elif case == "tiny":
        x = torch.exp(torch.rand(x.shape, generator=g) * (math.log(1e-4) - math.log(1e-6)) + math.log(1e-6)) * torch.sign(torch.randn(x.shape, generator=g))
        b = None; slope = 1.0
    return x.cuda(), w.cuda(), (b.cuda() if b is not None else None), slope


def reference(x, w, b, G, slope):
    """(y64, bound) on the device"""
    K = 9 * w.shape[1]
    x64, w64 = x.double(), w.double()
    pre = F.conv2d(x64, w64, None, 1, 1, 1, G)
    s1 = F.conv2d(x64.abs(), w64.abs(), None, 1, 1, 1, G)
    s2 = F.conv2d(torch.ones_like(x64), w64.abs(), None, 1, 1, 1, G)
    s3 = torch.zeros_like(pre)
    if b is not None:
        pre = pre + b.double()[None, :, None, None]; s3 = s3 + b.double().abs()[None, :, None, None]
    return F.leaky_relu(pre, slope), 2.0 ** -23 * max(8.0, math.sqrt(K)) * s1 + 2.0 ** -34 * s2 + 2.0 ** -23 * s3


def run_split(ops, x, w, b, G, slope):
    from vido_slam_amd.nets.ops import pack_gconv3x3_hs
    bb = b if b is not None else torch.zeros(w.shape[0], device=x.device)
    return ops.gconv3x3_hs_bias_act(x, pack_gconv3x3_hs(w.cpu(), G).cuda(), bb, G, slope)


def run_fp32(ops, x, w, b, G, slope):
    from vido_slam_amd.nets.ops import pack_gconv3x3
    bb = b if b is not None else torch.zeros(w.shape[0], device=x.device)
    return ops.gconv3x3_bias_act(x, pack_gconv3x3(w.cpu(), G).cuda(), bb, G, slope)


def measure(y, y64, bound):
    q = (y.double() - y64).abs() / bound.clamp_min(1e-300)
    return float(q.max()), float(q.pow(2).mean().sqrt())


def check(ops, shape, case, seed):
    G, cpg, H, W = shape
    assert ops.gconv3x3_hs_supported(H, W, cpg, cpg)
    x, w, b, slope = make_case(shape, case, seed)
    y64, bound = reference(x, w, b, G, slope)
    yf = run_fp32(ops, x, w, b, G, slope)
    mf, rf = measure(yf, y64, bound)
    ys = run_split(ops, x, w, b, G, slope)
    assert ys.shape == yf.shape == y64.shape
    ms, rs = measure(ys, y64, bound)
    print("gconv3x3_hs %s %s: max %.3f rms %.4f of the bound | fp32 kernel: max %.3f rms %.4f | ratio max %.2f rms %.2f" % (case, shape, ms, rs, mf, rf, ms / max(mf, 1e-30), rs / max(rf, 1e-30)))
    fails = []
    if not (ms <= 1.0):
        fails.append(("split-fp16 outside the bound", ms))
    if case in ("gauss", "x300") and not (ms <= 1.5 * mf and rs <= 1.5 * rf):
        fails.append(("split-fp16 noisier than 1.5x the fp32 kernel", ms, mf, rs, rf))
    torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0
    assert not fails, (shape, case, fails)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d@%dx%d" % s)
def test_small_shapes_within_the_elementwise_bound(vido, ops, shape, case):
    check(ops, shape, case, 100 * SMALL.index(shape) + CASES.index(case))


@pytest.mark.parametrize("shape", WIDE, ids=lambda s: "%dx%d@%dx%d" % s)
def test_full_row_width_within_the_elementwise_bound(vido, ops, shape):
    check(ops, shape, "gauss", 700 + shape[1])


@pytest.fixture(scope="module", params=WORKLOAD, ids=lambda s: "%dx%d@%dx%d" % s)
def full(request, ops):
    """(shape, x, packed weight, bias, slope, y of one run) at a workload shape: computed once, left unchanged"""
    from vido_slam_amd.nets.ops import pack_gconv3x3_hs
    shape = request.param
    x, w, b, slope = make_case(shape, "gauss", 900 + shape[1])
    wp = pack_gconv3x3_hs(w.cpu(), shape[0]).cuda()
    y = ops.gconv3x3_hs_bias_act(x, wp, b, shape[0], slope).clone()
    return shape, x, wp, b, slope, y


def test_workload_shapes_supported_same_bits_every_run_and_in_a_captured_graph(vido, ops, full):
    shape, x, wp, b, slope, y0 = full
    G, cpg, H, W = shape
    assert ops.gconv3x3_hs_supported(H, W, cpg, cpg), "the detector's layer1 / layer2 shapes are the kernel's reason to exist"
    assert bool(torch.isfinite(y0).all()) and float(y0.abs().max()) > 0
    assert torch.equal(ops.gconv3x3_hs_bias_act(x, wp, b, G, slope), y0)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.gconv3x3_hs_bias_act(x, wp, b, G, slope)                     # warm-up on the capture stream
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            yg = ops.gconv3x3_hs_bias_act(x, wp, b, G, slope)
    torch.cuda.current_stream().wait_stream(st)
    yg.zero_()
    gr.replay(); torch.cuda.synchronize()
    assert torch.equal(yg, y0)
    assert ops.conv1x1_range_flag(reset=True) == 0


def test_workload_shapes_rows_of_a_crop_have_the_full_run_s_bits(vido, ops, full):
    """Rows 0 .. 38 of a run on the first 40 input rows, and the inner rows of a run on a slab from the middle with one halo row each side, equal the full run's: other items,
    other rounds, other ring slots, the same sums."""
    shape, x, wp, b, slope, y0 = full
    G, cpg, H, W = shape
    yt = ops.gconv3x3_hs_bias_act(x[:, :, :40].contiguous(), wp, b, G, slope)
    assert torch.equal(yt[:, :, :39], y0[:, :, :39])
    assert not torch.equal(yt[:, :, 39], y0[:, :, 39]), "row 39 sees the crop's lower edge"
    lo, hi = H // 2 - 17, H // 2 + 14                                    # output rows lo .. hi - 1 from input rows lo - 1 .. hi
    ym = ops.gconv3x3_hs_bias_act(x[:, :, lo - 1:hi + 1].contiguous(), wp, b, G, slope)
    assert torch.equal(ym[:, :, 1:-1], y0[:, :, lo:hi])
    torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0


def test_supported_shapes(vido, ops):
    s = ops.gconv3x3_hs_supported
    assert s(200, 272, 8, 8) and s(100, 136, 16, 16) and s(1, 1, 8, 8) and s(7, 9, 16, 16) and s(3, 957, 8, 8) and s(3, 445, 16, 16)
    assert not s(3, 958, 8, 8) and not s(3, 446, 16, 16)                 # the ring of a round no longer fits half a CU's LDS
    assert not s(50, 68, 32, 32) and not s(50, 68, 8, 16) and not s(50, 68, 4, 4) and not s(0, 68, 8, 8)
    assert not ops.gconv3x3_h_supported(50, 68, 16, 16)                  # the 32 / 64 kernel keeps declining these
    from vido_slam_amd.nets.ops import pack_gconv3x3_hs
    with pytest.raises(vido.VidoError):                                  # the entry point refuses what supported() refuses
        ops.gconv3x3_hs_bias_act(torch.zeros(1, 32, 2, 500, device="cuda"), pack_gconv3x3_hs(torch.zeros(32, 16, 3, 3), 2).cuda(), torch.zeros(32, device="cuda"), 2, 0.0)


def test_range_flag_and_range_safe(vido, ops):
    """One activation of 70 000 raises the flag of the context that ran the launch and of no other; inside range_safe the dispatcher launches the fp32 kernel: its bits, flag down."""
    from vido_slam_amd.nets.ops import HipOps, pack_gconv3x3, pack_gconv3x3_hs, range_safe
    shape = (3, 8, 17, 20)
    x, w, b, slope = make_case(shape, "gauss", 5)
    x[0, 10, 9, 13] = 70000.0
    wp, wphs = pack_gconv3x3(w.cpu(), 3).cuda(), pack_gconv3x3_hs(w.cpu(), 3).cuda()
    ctx2 = vido.Context()
    try:
        ops2 = HipOps(ctx2)
        ops.conv1x1_range_flag(reset=True); ops2.conv1x1_range_flag(reset=True)
        for first, second in ((ops, ops2), (ops2, ops)):
            first.gconv3x3_conv(x, wp, None, b, 3, slope, w_packed_hs=wphs); torch.cuda.synchronize()
            assert second.conv1x1_range_flag(reset=True) == 0
            assert first.conv1x1_range_flag(reset=True) == 1
            assert first.conv1x1_range_flag(reset=True) == 0
    finally:
        ctx2.close()
    for v in (65504.0, math.inf, math.nan):
        xe = x.clone(); xe[0, 10, 9, 13] = v
        ops.gconv3x3_hs_bias_act(xe, wphs, b, 3, slope); torch.cuda.synchronize()
        assert ops.conv1x1_range_flag(reset=True) == 1, v
    xe = x.clone(); xe[0, 10, 9, 13] = 65000.0
    ops.gconv3x3_hs_bias_act(xe, wphs, b, 3, slope); torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0, "65000 is inside fp16's range"
    yf = ops.gconv3x3_bias_act(x, wp, b, 3, slope)
    with range_safe(ops):
        assert ops.range_safe_active
        ys = ops.gconv3x3_conv(x, wp, None, b, 3, slope, w_packed_hs=wphs)
    torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0, "a split-fp16 launch happened inside range_safe"
    assert torch.equal(ys, yf)
    assert bool(torch.isfinite(ys).all())                                # fp32's range: 70 000 is an ordinary activation there


def test_dispatch_falls_back_to_the_fp32_kernel(vido, ops, monkeypatch):
    """gconv3x3_conv runs the new kernel only with w_packed_hs given, no input bias, split arithmetic and both switches on; everything else gets gconv3x3_bias_act's bits."""
    import vido_slam_amd.nets.ops as O
    shape = (2, 8, 7, 9)
    x, w, b, slope = make_case(shape, "gauss", 6)
    wp, wphs = O.pack_gconv3x3(w.cpu(), 2).cuda(), O.pack_gconv3x3_hs(w.cpu(), 2).cuda()
    assert O.pack_gconv3x3_h(w.cpu(), 2) is None
    yf = ops.gconv3x3_bias_act(x, wp, b, 2, slope)
    ys = ops.gconv3x3_hs_bias_act(x, wphs, b, 2, slope)
    assert not torch.equal(ys, yf), "the two arithmetics should differ in some last bit on 1008 outputs"
    monkeypatch.setattr(O, "_GCONV_H", True); monkeypatch.setattr(O, "_GCONV_HS", True)
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, w_packed_hs=wphs), ys)
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, None, wphs), ys)
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope), yf)
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, w_packed_hs=None), yf)
    ib = torch.randn(16, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, in_bias=ib, w_packed_hs=wphs), ops.gconv3x3_bias_act(x, wp, b, 2, slope, in_bias=ib))
    prev = ops.conv1x1_set_arith(1)
    try:
        assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, w_packed_hs=wphs), yf)
    finally:
        ops.conv1x1_set_arith(prev)
    for h, hs in ((False, True), (True, False), (False, False)):         # what VIDO_GCONV_H=0 / VIDO_GCONV_HS=0 set at import
        monkeypatch.setattr(O, "_GCONV_H", h); monkeypatch.setattr(O, "_GCONV_HS", hs)
        assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, w_packed_hs=wphs), yf), (h, hs)
    monkeypatch.setattr(O, "_GCONV_H", True); monkeypatch.setattr(O, "_GCONV_HS", True)
    assert torch.equal(ops.gconv3x3_conv(x, wp, None, b, 2, slope, w_packed_hs=wphs), ys)
    # VIDO_GCONV_HS=0 leaves the 32 / 64 kernel where it was
    shape32 = (2, 32, 7, 9)
    x3, w3, b3, _ = make_case(shape32, "gauss", 7)
    w3p, w3ph = O.pack_gconv3x3(w3.cpu(), 2).cuda(), O.pack_gconv3x3_h(w3.cpu(), 2).cuda()
    monkeypatch.setattr(O, "_GCONV_HS", False)
    assert torch.equal(ops.gconv3x3_conv(x3, w3p, w3ph, b3, 2, 0.0), ops.gconv3x3_h_bias_act(x3, w3ph, b3, 2, 0.0))
    torch.cuda.synchronize()
    assert ops.conv1x1_range_flag(reset=True) == 0


def test_reads_and_writes_stay_inside_the_tensors(vido, ops):
    """x and y are views in the middle of NaN-filled buffers: the output is finite and within the bound, the bytes around y are untouched, the flag stays down."""
    from vido_slam_amd.nets.ops import pack_gconv3x3_hs
    for shape in ((3, 8, 17, 20), (2, 16, 9, 12), (3, 8, 3, 140)):
        G, cpg, H, W = shape
        x, w, b, slope = make_case(shape, "gauss", 7)
        n = x.numel(); pad = 4099
        xbuf = torch.full((n + 2 * pad,), math.nan, device="cuda"); xbuf[pad:pad + n] = x.reshape(-1)
        ybuf = torch.full((n + 2 * pad,), math.nan, device="cuda")
        wphs = pack_gconv3x3_hs(w.cpu(), G).cuda()
        ops._adopt_stream()
        xv, yv = xbuf[pad:pad + n], ybuf[pad:pad + n]
        ops.ctx._check(ops.ctx.lib.vido_gconv3x3_hs_bias_act(ops.ctx.h, C.c_void_p(xv.data_ptr()), C.c_void_p(wphs.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(yv.data_ptr()),
                                                             G, cpg, cpg, H, W, C.c_float(slope)))
        torch.cuda.synchronize()
        assert ops.conv1x1_range_flag(reset=True) == 0, "a NaN outside x was read"
        assert bool(torch.isnan(ybuf[:pad]).all()) and bool(torch.isnan(ybuf[pad + n:]).all()), "a store outside y"
        y = yv.reshape(x.shape)
        assert bool(torch.isfinite(y).all())
        y64, bound = reference(x, w, b, G, slope)
        assert measure(y, y64, bound)[0] <= 1.0


def test_groups_do_not_mix(vido, ops):
    """Changing the input of group 1 leaves the outputs of groups 0 and 2 bit-identical (and changes group 1's)."""
    for shape in ((3, 8, 17, 20), (3, 16, 5, 33)):
        cpg = shape[1]
        x, w, b, slope = make_case(shape, "gauss", 8)
        y0 = run_split(ops, x, w, b, 3, slope)
        x2 = x.clone(); x2[:, cpg:2 * cpg] = x2[:, cpg:2 * cpg] * 1.5 + 0.25
        y1 = run_split(ops, x2, w, b, 3, slope)
        assert torch.equal(y0[:, :cpg], y1[:, :cpg]) and torch.equal(y0[:, 2 * cpg:], y1[:, 2 * cpg:])
        assert not torch.equal(y0[:, cpg:2 * cpg], y1[:, cpg:2 * cpg])
