"""csrc/stem.hip on the MI355X: the detector's stem — 7x7 stride-2 convolution + bias + ReLU + 3x3 stride-2 max-pool — as one launch, against the same expression in
float64 on the device.  Yardstick: the expression in fp32 through torch (the path the launch replaces).  Bound: the launch's max and rms error against float64 are at most
2 x the fp32 torch path's on the same inputs — the factor covers another summation order over K = 147 fp32 products, nothing more.

Shapes (pooled tile of the kernel: 7 x 8): 3x7x7 (one workgroup, almost every staged element is padding), 3x37x45 and 3x70x50 (odd / even convolution sizes, pooled sizes
that are no multiple of the tile), 3x64x96, 3x30x34 (pooled 8 x 9: one tile + 1 in each direction)."""
import pytest
import torch
import torch.nn.functional as F
from vido_slam_amd import nets

pytestmark = pytest.mark.gpu
SHAPES = [(7, 7), (37, 45), (70, 50), (64, 96), (30, 34)]


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


def _chain(x, w, b):
    return F.max_pool2d(F.relu(F.conv2d(x, w, None, 2, 3) + b[None, :, None, None]), 3, 2, 1)


def _fused(ops, x, w, b):
    from vido_slam_amd.nets.ops import pack_stem7x7
    return ops.stem7x7s2_pool(x, pack_stem7x7(w).cuda(), b)


def _errors(y, ref):
    d = y.double() - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


def _check(ops, x, w, b, what):
    ref = _chain(x.double(), w.double(), b.double())
    y = _fused(ops, x, w, b); y32 = _chain(x, w, b)
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    (mx, rms), (mx32, rms32) = _errors(y, ref), _errors(y32, ref)
    print("stem %s: fused max %.3e rms %.3e | fp32 torch max %.3e rms %.3e | scale %.3e" % (what, mx, rms, mx32, rms32, float(ref.abs().max())))
    assert bool(torch.isfinite(y).all()) and float(y.min()) >= 0.0, what
    assert mx <= 2.0 * mx32 and rms <= 2.0 * rms32, (what, mx, mx32, rms, rms32)


@pytest.mark.parametrize("H,W", SHAPES)
def test_stem_fused_against_float64(vido, ctx, H, W):
    """the image in area_feed's range (about +-128) and as unit Gaussians; weights at the scale of a folded stem"""
    ops = nets.HipOps(ctx)
    g = torch.Generator().manual_seed(H * 131 + W)
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).cuda(); b = torch.randn(64, generator=g).cuda()
    for what, x in (("%dx%d +-128" % (H, W), torch.rand(1, 3, H, W, generator=g) * 256 - 128), ("%dx%d gauss" % (H, W), torch.randn(1, 3, H, W, generator=g))):
        _check(ops, x.cuda(), w, b, what)


@pytest.mark.parametrize("H,W", SHAPES)
def test_stem_fused_bias_cases(vido, ctx, H, W):
    ops = nets.HipOps(ctx)
    g = torch.Generator().manual_seed(H * 17 + W)
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).cuda()
    x = (torch.rand(1, 3, H, W, generator=g) * 256 - 128).cuda()
    pre = F.conv2d(x.double(), w.double(), None, 2, 3)
    # every pre-activation value negative: the output is exactly zero (a padded element, a stale LDS word or a -inf that reached the output would show)
    b = (-pre.amax(dim=(0, 2, 3)) - 1.0).float()
    y = _fused(ops, x, w, b)
    assert torch.equal(y, torch.zeros_like(y)), (H, W, float(y.abs().max()))
    # the border values are the maxima: a non-negative image under non-positive weights makes every product <= 0, so a convolution output that sees the zero padding is
    # larger than its inner neighbours, and one OUTSIDE the map (computed from even fewer real pixels) would be larger still: it must not win its pool window.  The bias
    # lifts every value above zero so that the ReLU hides nothing.
    xp = (torch.rand(1, 3, H, W, generator=g) * 128).cuda(); wn = -w.abs()
    bp = (-F.conv2d(xp.double(), wn.double(), None, 2, 3).amin(dim=(0, 2, 3)) + 1.0).float()
    _check(ops, xp, wn, bp, "%dx%d border maxima" % (H, W))


def test_stem_module_takes_the_fused_launch_for_one_image_only(vido, ctx, monkeypatch):
    """_Stem after fold_batchnorm: the fused launch against the path behind VIDO_NO_STEM_FUSED=1 (library convolution, bias + ReLU pass, max-pool) on 1x3x96x128, the same
    bound; a batch of two keeps the present path."""
    from vido_slam_amd.nets.maskrcnn import _Stem
    ops = nets.HipOps(ctx)
    stem = _Stem(64).eval().cuda(); nets.fill_deterministic(stem, 5)
    assert nets.fold_batchnorm(stem, ops) == 1
    calls = []
    real = ops.stem7x7s2_pool
    monkeypatch.setattr(ops, "stem7x7s2_pool", lambda *a: (calls.append(1), real(*a))[1])
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 3, 96, 128, generator=g) * 256 - 128).cuda()
    with torch.no_grad():
        y1 = stem(x[:1]); assert len(calls) == 1
        y2 = stem(x); assert len(calls) == 1
        monkeypatch.setenv("VIDO_NO_STEM_FUSED", "1")
        y1n = stem(x[:1]); y2n = stem(x); assert len(calls) == 1
        ref = _chain(x[:1].double(), stem._w1.double(), stem._b1.double())
    assert torch.equal(y2, y2n) and tuple(y1.shape) == tuple(y1n.shape) == (1, 64, 24, 32)
    (mx, rms), (mx32, rms32) = _errors(y1, ref), _errors(y1n, ref)
    print("stem module 96x128: fused max %.3e rms %.3e | present path max %.3e rms %.3e" % (mx, rms, mx32, rms32))
    assert mx <= 2.0 * mx32 and rms <= 2.0 * rms32, (mx, mx32, rms, rms32)
