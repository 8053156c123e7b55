"""csrc/convsmall.hip::k_conv1x1_skinny on the MI355X: the depth of its load batches (VIDO_SKINNY_DEPTH, 16 by default for up to 32 output channels) changes how many
k-pairs a wave has in flight, not the order in which they are accumulated: every depth must give the 4-deep form's bits.  Channel-pair counts that are no multiple of 4, 8
or 16 (the clamped tail) and the RPN's 128; one and several 32-channel output blocks; position counts around the 32 of a wave and the 128 of a workgroup."""
import pytest
import torch
from vido_slam_amd import nets

pytestmark = pytest.mark.gpu
HW = [(1, 1), (1, 31), (3, 11), (1, 127), (13, 17), (40, 85)]                # 1, 31, 33, 127, 221, 3400 positions
COUT = [1, 15, 32, 33, 128]


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


@pytest.mark.parametrize("cin", [2, 6, 34, 130, 256])
def test_every_depth_gives_the_bits_of_the_four_deep_form(vido, ctx, cin, monkeypatch):
    from vido_slam_amd.nets.ops import pack_conv1x1_skinny
    ops = nets.HipOps(ctx)
    g = torch.Generator().manual_seed(cin)
    for cout in COUT:
        wp = pack_conv1x1_skinny(torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).cuda(); b = torch.randn(cout, generator=g).cuda()
        for H, W in HW:
            x = torch.randn(1, cin, H, W, generator=g).cuda(); r = torch.randn(1, cout, H, W, generator=g).cuda()
            variants = [(b, slope, res) for slope in (0.0, 0.1, 1.0) for res in (None, r)] + [(None, 1.0, None)]
            out = {}
            for depth in ("4", "8", "16", None):
                if depth is None:
                    monkeypatch.delenv("VIDO_SKINNY_DEPTH", raising=False)
                else:
                    monkeypatch.setenv("VIDO_SKINNY_DEPTH", depth)
                out[depth] = [ops.conv1x1_skinny(x, wp, bias, cout, slope, res) for bias, slope, res in variants]
            for depth in ("8", "16", None):
                for y, y4, v in zip(out[depth], out["4"], variants):
                    assert torch.equal(y, y4), (cin, cout, H, W, depth, v[1], v[2] is not None, v[0] is None)
            ref = torch.nn.functional.conv2d(x.double(), _unpack(wp, cout, cin).double(), b.double())      # the 4-deep form itself is right
            assert float((out["4"][4][0].double() - ref[0]).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max())), (cin, cout, H, W)


def _unpack(wp, cout, cin):
    """inverse of pack_conv1x1_skinny: [cout / 32][cin / 2][64] -> [cout, cin, 1, 1]"""
    cbn = wp.shape[0]
    return wp.reshape(cbn, cin // 2, 2, 32).permute(0, 3, 1, 2).reshape(cbn * 32, cin)[:cout].reshape(cout, cin, 1, 1)


def test_a_depth_without_a_form_is_an_error(vido, ctx, monkeypatch):
    from vido_slam_amd.nets.ops import pack_conv1x1_skinny
    ops = nets.HipOps(ctx)
    monkeypatch.setenv("VIDO_SKINNY_DEPTH", "5")
    with pytest.raises(vido.VidoError):
        ops.conv1x1_skinny(torch.zeros(1, 4, 2, 2, device="cuda"), pack_conv1x1_skinny(torch.zeros(3, 4, 1, 1)).cuda(), None, 3, 1.0)


def test_rpn_head_default_depth_against_the_four_deep_form(vido, ctx, monkeypatch):
    from vido_slam_amd.nets.maskrcnn import _RPNHead
    ops = nets.HipOps(ctx)
    head = _RPNHead(256, 3).eval().cuda(); nets.fill_deterministic(head, 11); head._ops = ops
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(1, 256, h, w, generator=g).cuda() for h, w in ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))]
    with torch.no_grad():
        monkeypatch.delenv("VIDO_SKINNY_DEPTH", raising=False)
        obj, box = head(feats)
        monkeypatch.setenv("VIDO_SKINNY_DEPTH", "4")
        obj4, box4 = head(feats)
    assert hasattr(head, "_head_w")                                           # (the skinny launches ran, not the library's two convolutions)
    for a, b in zip(obj + box, obj4 + box4):
        assert torch.equal(a, b)
    assert [tuple(o.shape) for o in obj] == [(1, 3, 16, 20), (1, 3, 8, 10), (1, 3, 4, 5), (1, 3, 2, 3), (1, 3, 1, 2)] and tuple(box[0].shape) == (1, 12, 16, 20)
