"""MI355X: vido_dis_flow (csrc/disflow.hip: k_dis_ingest, k_dis_down, k_dis_patch, k_dis_densify) against the numpy / Python-integer statement
(tests/refimpl/dis_flow_np.py): q8, stats and flow bit for bit, no tolerance anywhere.  Shapes: 16 x 16 (the coarsest level is a single patch), 64 x 64, 73 x 50 (edge-aligned
patches on both axes, halves through odd sizes), 201 x 151 at two depths, one 640 x 480 Scene3D pair at the defaults; hostile content at 64 x 64; strides, channels, the
host and the device form, sizes in turn on one context, every refusal.  The context is configured for 64 x 64: the op does not depend on that."""
import ctypes as C
import numpy as np
import pytest

from refimpl import dis_flow_np as D

pytestmark = pytest.mark.gpu

NAMES = ("flow", "q8", "stats")


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _pair(vido, w, h, seed, d=(300, -200)):
    """Two views of one canvas: the second resampled by the statement's own bilinear form at d / 256 px, so the flow is a known sub-pixel translation"""
    canvas = vido.synth.make_canvas(h + 6, w + 6, seed, n_rect=max(4, w * h // 1500))
    return np.ascontiguousarray(canvas[3:3 + h, 3:3 + w]), np.ascontiguousarray(D.resample(canvas, -d[0], -d[1])[3:3 + h, 3:3 + w])


def _same(got, want):
    assert len(got) == len(want) == 3
    for g, w_, name in zip(got, want, NAMES):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if not np.array_equal(g, w_):
            bad = np.argwhere(g != w_)
            assert False, (name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])
    assert np.array_equal(got[0], got[1].astype(np.float32) / np.float32(256))              # flow == q8 / 256 exactly


@pytest.mark.parametrize("w,h,coarsest", [(16, 16, 1), (64, 64, 2), (73, 50, 2), (201, 151, 3), (201, 151, 4)])
def test_bit_equal_at_the_small_shapes(vido, ctx, w, h, coarsest):
    a, b = _pair(vido, w, h, seed=w + coarsest)
    want = D.dis_flow(a, b, coarsest=coarsest)
    print("dis_flow %d x %d coarsest %d: stats %s, |q8| max %d, median %s" % (w, h, coarsest, want[2].tolist(), np.abs(want[1]).max(), np.median(want[1].reshape(-1, 2), 0).tolist()))
    assert want[2][0] > 0 and want[1].any()
    _same(ctx.dis_flow(a, b, coarsest=coarsest), want)


def test_bit_equal_on_a_scene3d_pair_at_the_defaults(vido, ctx):
    sc = vido.synth.Scene3D()
    g1, g2 = sc.frame(1)[0], sc.frame(2)[0]
    want = D.dis_flow(g1, g2, **D.DEFAULTS)
    assert want[2][0] > 20000 and want[2][2] > 0
    _same(ctx.dis_flow(g1, g2), want)


def _checker(n=64):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((((yy >> 1) + (xx >> 1)) & 1) * 255).astype(np.uint8)


def test_hostile_content(vido, ctx):
    rng = np.random.RandomState(8)
    c = _checker(); noise = [rng.randint(0, 256, (64, 64)).astype(np.uint8) for _ in range(2)]
    tex = vido.synth.make_canvas(64, 88, 12, n_rect=30)
    a, b = _pair(vido, 64, 64, seed=21)
    cases = [("constant", np.full((64, 64), 200, np.uint8), noise[0], dict(coarsest=2)),
             ("checker against inverse", c, (255 - c).astype(np.uint8), dict(coarsest=2)),
             ("checker against shifted checker", c, np.roll(c, 1, axis=1), dict(coarsest=0, iters=16, max_shift_q8=2048)),
             ("noise against unrelated noise", noise[0], noise[1], dict(coarsest=2, iters=16)),
             ("12-px shift, window 1 px", np.ascontiguousarray(tex[:, 12:76]), np.ascontiguousarray(tex[:, 0:64]), dict(coarsest=0, max_shift_q8=256)),
             ("iters 1", a, b, dict(coarsest=2, iters=1)), ("iters 16", a, b, dict(coarsest=2, iters=16)),
             ("max_shift_q8 0", a, b, dict(coarsest=2, max_shift_q8=0)), ("max_shift_q8 2048", a, b, dict(coarsest=2, max_shift_q8=2048)),
             ("max_shift_q8 255", a, b, dict(coarsest=2, max_shift_q8=255)), ("min_eig", a, b, dict(coarsest=2, min_eig=2000000)),
             ("largest min_eig", a, b, dict(coarsest=1, min_eig=2 ** 31 - 1))]
    seen = np.zeros(4, np.int64)
    for name, i0, i1, kw in cases:
        want = D.dis_flow(i0, i1, **kw)
        print("%-32s stats %s" % (name, want[2].tolist()))
        seen += want[2]
        _same(ctx.dis_flow(i0, i1, **kw), want)
    assert (seen > 0).all()
    assert D.dis_flow(noise[0], noise[1], coarsest=2, iters=16)[2][2] > 0                   # rejections
    assert D.dis_flow(cases[0][1], cases[0][2], coarsest=2)[2].tolist() == [0, D.n_patches(64, 64, 2), 0, 0]


def test_row_stride_and_channels(vido, ctx):
    rng = np.random.RandomState(4)
    a, b = _pair(vido, 73, 50, seed=5)
    want = D.dis_flow(a, b, coarsest=2)
    wide = [np.full((50, 96), 7, np.uint8) for _ in range(2)]
    wide[0][:, :73] = a; wide[1][:, :73] = b
    _same(ctx.dis_flow(wide[0][:, :73], wide[1][:, :73], coarsest=2), want)                 # stride 96 > width 73
    for cn in (3, 4):
        c0, c1 = rng.randint(0, 256, (50, 73, cn)).astype(np.uint8), rng.randint(0, 256, (50, 73, cn)).astype(np.uint8)
        c1[..., :3] = c0[..., :3] // 2 + np.roll(c0[..., :3], 1, axis=1) // 2               # related content, channels that differ
        for order in (0, 1):
            w_ = D.dis_flow(c0, c1, coarsest=2, rgb_order=order)
            _same(ctx.dis_flow(c0, c1, coarsest=2, rgb_order=order), w_)
            _same(ctx.dis_flow(D.grey(c0, order).astype(np.uint8), D.grey(c1, order).astype(np.uint8), coarsest=2), w_)
        assert not np.array_equal(D.dis_flow(c0, c1, coarsest=2, rgb_order=0)[1], D.dis_flow(c0, c1, coarsest=2, rgb_order=1)[1])
        pad = [np.zeros((50, 73 * cn + 11), np.uint8) for _ in range(2)]                    # a colour row stride that is no multiple of the pixel
        pad[0][:, :73 * cn] = c0.reshape(50, -1); pad[1][:, :73 * cn] = c1.reshape(50, -1)
        v0 = np.lib.stride_tricks.as_strided(pad[0], (50, 73, cn), (pad[0].strides[0], cn, 1)); v1 = np.lib.stride_tricks.as_strided(pad[1], (50, 73, cn), (pad[1].strides[0], cn, 1))
        _same(ctx.dis_flow(v0, v1, coarsest=2, rgb_order=1), D.dis_flow(c0, c1, coarsest=2, rgb_order=1))


def test_device_form_equals_host_form_with_and_without_each_output(vido, ctx):
    import torch
    a, b = _pair(vido, 73, 50, seed=9)
    want = ctx.dis_flow(a, b, coarsest=2)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    shapes = ((50, 73, 2), (50, 73, 2), (4,)); dtypes = (torch.float32, torch.int32, torch.int32)
    for mask in (1, 2, 4, 3, 5, 6, 7):
        outs = [torch.full(s, -77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
        torch.cuda.synchronize()
        ptrs = [o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)]
        ctx.dis_flow_device(ta.data_ptr(), tb.data_ptr(), 1, 73, 73, 50, coarsest=2, flow_ptr=ptrs[0], q8_ptr=ptrs[1], stats_ptr=ptrs[2])
        ctx.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), want[i]) if mask >> i & 1 else bool((o == -77).all()), (mask, i)


def test_sizes_in_turn_on_one_context(vido, ctx):
    a, b = _pair(vido, 64, 64, seed=31); c, d = _pair(vido, 201, 151, seed=32); e, f = _pair(vido, 16, 16, seed=33)
    first = ctx.dis_flow(a, b, coarsest=2)
    _same(first, D.dis_flow(a, b, coarsest=2))
    _same(ctx.dis_flow(c, d, coarsest=4), D.dis_flow(c, d, coarsest=4))
    _same(ctx.dis_flow(e, f, coarsest=1), D.dis_flow(e, f, coarsest=1))
    _same(ctx.dis_flow(a, b, coarsest=2), first)
    _same(ctx.dis_flow(a, b, coarsest=0), D.dis_flow(a, b, coarsest=0))
    _same(ctx.dis_flow(a, b, coarsest=2), first)


def test_every_refusal_leaves_the_context_usable(vido, ctx):
    import torch
    a, b = _pair(vido, 64, 64, seed=41)
    good = ctx.dis_flow(a, b, coarsest=2)
    lib = ctx.lib; f = lib.vido_dis_flow
    flow = np.empty((64, 64, 2), np.float32); q8 = np.empty((64, 64, 2), np.int32); stats = np.empty(4, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(ctx.h).decode()
    call = lambda i0=P(a), i1=P(b), cn=1, order=0, stride=64, w=64, h=64, L=2, iters=6, shift=1024, eig=0, o=(P(flow), P(q8), P(stats)), dev=0: f(ctx.h, i0, i1, cn, order, stride, w, h, L, iters, shift, eig, *o, dev)
    assert call() == 0
    assert call(i0=None) == -1 and "image" in err()
    assert call(i1=None) == -1 and "image" in err()
    for w, h in ((15, 64), (64, 15), (4096, 64), (64, 4096), (0, 0), (-1, 64)):
        assert call(w=w, h=h, stride=max(w, 64)) == -1 and "size" in err()
    for cn in (0, 2, 5, -1):
        assert call(cn=cn, stride=64 * 8) == -1 and "channels" in err()
    assert call(stride=63) == -1 and "stride" in err()
    assert call(cn=3, stride=191) == -1 and "stride" in err()
    for L in (-1, 7, 4, 1 << 20):                                                           # 64 >> 4 = 4 < 8
        assert call(L=L) == -1 and "coarsest" in err()
    assert call(L=3) == 0
    for iters in (-1, 0, 17, 1 << 20):
        assert call(iters=iters) == -1 and "iters" in err()
    for shift in (-1, 2049, 1 << 20):
        assert call(shift=shift) == -1 and "max_shift_q8" in err()
    assert call(eig=-1) == -1 and "min_eig" in err()
    assert call(o=(None, None, None)) == -1 and "output" in err()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    t = [torch.zeros(64 * 64 * 2 + 1, dtype=torch.int32, device="cuda") for _ in range(3)]
    dp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    for k in range(3):                                                                      # device form, one misaligned output: refused before any launch
        o = tuple(dp(t[i], 2 if i == k else 0) for i in range(3))
        assert call(i0=dp(ta), i1=dp(tb), o=o, dev=1) == -1 and "aligned" in err()
    assert f(None, P(a), P(b), 1, 0, 64, 64, 64, 2, 6, 1024, 0, P(flow), P(q8), P(stats), 0) == -1
    with pytest.raises(vido.VidoError):
        ctx.dis_flow(a, b[:32])
    _same(ctx.dis_flow(a, b, coarsest=2), good)


def test_hipops_form_on_torch_tensors(vido, ctx):
    """HipOps.dis_flow on u8 device tensors, grey and BGR, on torch's current stream: equal to the host form; wrong device, dtype, shape or contiguity raises."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    a, b = _pair(vido, 73, 50, seed=51)
    ca, cb = np.ascontiguousarray(np.stack([a, np.roll(a, 1, 1), 255 - a], -1)), np.ascontiguousarray(np.stack([b, np.roll(b, 1, 1), 255 - b], -1))
    for i0, i1 in ((a, b), (ca, cb)):
        want = ctx.dis_flow(i0, i1, coarsest=2, iters=4)
        t0, t1 = torch.from_numpy(i0).cuda(), torch.from_numpy(i1).cuda()
        q8 = torch.full((50, 73, 2), -77, dtype=torch.int32, device="cuda"); stats = torch.full((4,), -77, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            flow = ops.dis_flow(t0, t1, q8=q8, stats=stats, coarsest=2, iters=4)
        side.synchronize()
        _same((flow.cpu().numpy(), q8.cpu().numpy(), stats.cpu().numpy()), want)
        out = torch.empty((50, 73, 2), dtype=torch.float32, device="cuda")
        assert ops.dis_flow(t0, t1, out=out, coarsest=2, iters=4) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0])
    t0, t1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    bad = [(t0.cpu(), t1, {}), (t0, t1.float(), {}), (t0, t1[:, :64].contiguous(), {}), (t0[:, ::2], t1[:, ::2], {}), (t0[None], t1[None], {}),
           (torch.from_numpy(np.stack([a, a], -1)).cuda(), torch.from_numpy(np.stack([b, b], -1)).cuda(), {}),
           (t0, t1, dict(out=torch.empty((50, 73), dtype=torch.float32, device="cuda"))), (t0, t1, dict(out=torch.empty((50, 73, 2), dtype=torch.float64, device="cuda"))),
           (t0, t1, dict(q8=torch.empty((50, 73, 2), dtype=torch.int64, device="cuda"))), (t0, t1, dict(stats=torch.empty((3,), dtype=torch.int32, device="cuda"))),
           (t0, t1, dict(out=torch.empty((50, 73, 2), dtype=torch.float32))), (t0, t1, dict(iters=17))]
    for x, y, kw in bad:
        with pytest.raises(vido.VidoError):
            ops.dis_flow(x, y, **kw)
    _same(ctx.dis_flow(a, b, coarsest=2), D.dis_flow(a, b, coarsest=2))
