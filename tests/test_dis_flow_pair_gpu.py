"""MI355X: vido_dis_flow_pair (csrc/disflow.hip with the direction as a grid dimension, then csrc/flowcheck.hip's k_flow_check) against the statements: the forward field
and counters equal tests/refimpl/dis_flow_np.py's dis_flow(a, b), the backward ones dis_flow(b, a), and the marked flow, the status and the check's counters equal
tests/refimpl/flow_consistency_np.py on those two fields — all bit for bit, and equal to Context.dis_flow called twice.  Shapes: 16 x 16, 64 x 64, 73 x 50 and 201 x 151
translation pairs, the same with an occluding square moved 3 px, 3-channel input with a padded stride, one 640 x 480 Scene3D pair at the defaults; the device form inside a
graph capture; vido_dis_flow after a pair call on one context (the scratch is shared); refusals."""
import ctypes as C
import numpy as np
import pytest

from refimpl import dis_flow_np as D
from refimpl import flow_consistency_np as F
from test_dis_flow_gpu import _pair

pytestmark = pytest.mark.gpu

NAMES = ("marked flow", "fwd_q8", "bwd_q8", "status", "stats")
SHAPES = [(16, 16, 1), (64, 64, 2), (73, 50, 2), (201, 151, 4)]


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _statement(a, b, alpha_q10=10, beta_q16=32768, **kw):
    """The pair op's five outputs from the two statements"""
    f, g = D.dis_flow(a, b, **kw), D.dis_flow(b, a, **kw)
    status, marked, cstats = F.flow_consistency(f[1], g[1], alpha_q10, beta_q16)
    return marked, f[1], g[1], status, np.concatenate([f[2], g[2], cstats]).astype(np.int32)


def _same(got, want):
    assert len(got) == len(want) == 5
    for g, w_, name in zip(got, want, NAMES):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if g.dtype == np.float32:
            g, w_ = g.view(np.uint32), w_.view(np.uint32)                                     # NaNs compare by their bits
        if not np.array_equal(g, w_):
            bad = np.argwhere(g != w_)
            assert False, (name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])


def _twice(ctx, a, b, alpha_q10=10, beta_q16=32768, **kw):
    """The same five outputs from Context.dis_flow called twice and Context.flow_consistency"""
    f, g = ctx.dis_flow(a, b, **kw), ctx.dis_flow(b, a, **kw)
    status, marked, cstats = ctx.flow_consistency(f[1], g[1], alpha_q10, beta_q16)
    return marked, f[1], g[1], status, np.concatenate([f[2], g[2], cstats])


def _occluded(vido, w, h, seed):
    """A translation pair with a textured square in front that moves 3 px against the background's (300, -200) / 256: the background beside it is covered in one image"""
    a, b = _pair(vido, w, h, seed=seed)
    s = max(6, min(w, h) // 4)
    sq = vido.synth.make_canvas(s, s, seed + 100, n_rect=6)
    a, b = a.copy(), b.copy()
    y0, x0 = h // 3, w // 3
    a[y0:y0 + s, x0:x0 + s] = sq; b[y0:y0 + s, x0 + 3:x0 + 3 + s] = sq
    return a, b


@pytest.mark.parametrize("w,h,coarsest", SHAPES)
def test_bit_equal_on_the_translation_pairs(vido, ctx, w, h, coarsest):
    a, b = _pair(vido, w, h, seed=w + coarsest)
    want = _statement(a, b, coarsest=coarsest)
    print("dis_flow_pair %d x %d coarsest %d: stats %s" % (w, h, coarsest, want[4].tolist()))
    assert want[4][0] > 0 and want[4][4] > 0 and want[4][8] > 0 and want[4][10] > 0
    _same(ctx.dis_flow_pair(a, b, coarsest=coarsest), want)
    _same(_twice(ctx, a, b, coarsest=coarsest), want)


@pytest.mark.parametrize("w,h,coarsest", SHAPES)
def test_bit_equal_with_an_occluding_square(vido, ctx, w, h, coarsest):
    a, b = _occluded(vido, w, h, seed=2 * w + coarsest)
    want = _statement(a, b, coarsest=coarsest)
    print("dis_flow_pair, occluding square, %d x %d coarsest %d: stats %s" % (w, h, coarsest, want[4].tolist()))
    _same(ctx.dis_flow_pair(a, b, coarsest=coarsest), want)
    _same(_twice(ctx, a, b, coarsest=coarsest), want)
    for alpha, beta in ((0, 0), (1024, 1 << 30)):                                             # the check's parameters reach the check
        _same(ctx.dis_flow_pair(a, b, coarsest=coarsest, alpha_q10=alpha, beta_q16=beta), _statement(a, b, alpha, beta, coarsest=coarsest))


def test_three_channels_with_a_padded_stride(vido, ctx):
    rng = np.random.RandomState(4)
    c0 = rng.randint(0, 256, (50, 73, 3)).astype(np.uint8)
    c1 = (c0 // 2 + np.roll(c0, 1, axis=1) // 2).astype(np.uint8)                             # related content, channels that differ
    pad = [np.zeros((50, 73 * 3 + 11), np.uint8) for _ in range(2)]                           # a colour row stride that is no multiple of the pixel
    pad[0][:, :219] = c0.reshape(50, -1); pad[1][:, :219] = c1.reshape(50, -1)
    v0 = np.lib.stride_tricks.as_strided(pad[0], (50, 73, 3), (pad[0].strides[0], 3, 1)); v1 = np.lib.stride_tricks.as_strided(pad[1], (50, 73, 3), (pad[1].strides[0], 3, 1))
    for order in (0, 1):
        want = _statement(c0, c1, coarsest=2, rgb_order=order)
        _same(ctx.dis_flow_pair(v0, v1, coarsest=2, rgb_order=order), want)
        _same(ctx.dis_flow_pair(c0, c1, coarsest=2, rgb_order=order), want)


def test_bit_equal_on_a_scene3d_pair_at_the_defaults(vido, ctx):
    sc = vido.synth.Scene3D()
    g1, g2 = sc.frame(1)[0], sc.frame(2)[0]
    want = _statement(g1, g2, **D.DEFAULTS)
    print("dis_flow_pair, Scene3D 640 x 480 at the defaults: stats %s" % want[4].tolist())
    assert (want[4][8:11] > 0).all()
    _same(ctx.dis_flow_pair(g1, g2), want)


def test_device_form_in_a_graph_capture_and_without_outputs(vido, ctx):
    import torch
    pairs = [_pair(vido, 73, 50, seed=9), _occluded(vido, 73, 50, seed=10), _pair(vido, 73, 50, seed=11, d=(-150, 420))]
    wants = [ctx.dis_flow_pair(a, b, coarsest=2) for a, b in pairs]
    ta, tb = torch.from_numpy(pairs[0][0]).cuda(), torch.from_numpy(pairs[0][1]).cuda()
    shapes = ((50, 73, 2), (50, 73, 2), (50, 73, 2), (50, 73), (12,)); dtypes = (torch.float32, torch.int32, torch.int32, torch.uint8, torch.int32)
    view = lambda i, x: x.view(np.uint32) if i == 0 else x
    for mask in (1, 2, 4, 8, 16, 9, 22, 31):                                                  # each output alone, and without the q8 fields (the check then reads the scratch's)
        outs = [torch.full(s, 77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
        torch.cuda.synchronize()
        ptrs = [o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)]
        ctx.dis_flow_pair_device(ta.data_ptr(), tb.data_ptr(), 1, 73, 73, 50, coarsest=2, flow_ptr=ptrs[0], fwd_ptr=ptrs[1], bwd_ptr=ptrs[2], status_ptr=ptrs[3], stats_ptr=ptrs[4])
        ctx.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(view(i, o.cpu().numpy()), view(i, wants[0][i])) if mask >> i & 1 else bool((o == 77).all()), (mask, i)
    # captured on torch's capture stream, which the context adopts for the capture; replayed with new image contents
    outs = [torch.zeros(s, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
    adopt = lambda on: ctx._check(ctx.lib.vido_set_stream(ctx.h, C.c_void_p(torch.cuda.current_stream().cuda_stream) if on else None, 1 if on else 0))
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            adopt(True)
            ctx.dis_flow_pair_device(ta.data_ptr(), tb.data_ptr(), 1, 73, 73, 50, coarsest=2, flow_ptr=outs[0].data_ptr(), fwd_ptr=outs[1].data_ptr(), bwd_ptr=outs[2].data_ptr(),
                                     status_ptr=outs[3].data_ptr(), stats_ptr=outs[4].data_ptr())
    finally:
        adopt(False)
    for k in (1, 2, 0, 1):
        ta.copy_(torch.from_numpy(pairs[k][0])); tb.copy_(torch.from_numpy(pairs[k][1]))
        g.replay(); torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(view(i, o.cpu().numpy()), view(i, wants[k][i])), (k, NAMES[i])
    assert not np.array_equal(wants[0][3], wants[1][3]) and not np.array_equal(wants[1][1], wants[2][1])


def test_single_direction_call_after_a_pair_call_on_one_context(vido, ctx):
    a, b = _pair(vido, 201, 151, seed=32); c, d = _pair(vido, 64, 64, seed=31)
    def same3(got, want):
        for g, w_ in zip(got, want):
            assert g.dtype == w_.dtype and np.array_equal(g, w_)
    _same(ctx.dis_flow_pair(a, b, coarsest=4), _statement(a, b, coarsest=4))
    same3(ctx.dis_flow(a, b, coarsest=4), D.dis_flow(a, b, coarsest=4))                        # the scratch the pair call laid out, read under the one-direction layout
    same3(ctx.dis_flow(c, d, coarsest=2), D.dis_flow(c, d, coarsest=2))
    _same(ctx.dis_flow_pair(c, d, coarsest=2), _statement(c, d, coarsest=2))
    same3(ctx.dis_flow(b, a, coarsest=3), D.dis_flow(b, a, coarsest=3))
    _same(ctx.dis_flow_pair(a, b, coarsest=3), _statement(a, b, coarsest=3))


def test_every_refusal_leaves_the_context_usable(vido, ctx):
    import torch
    a, b = _pair(vido, 64, 64, seed=41)
    good = ctx.dis_flow_pair(a, b, coarsest=2)
    lib = ctx.lib; f = lib.vido_dis_flow_pair
    outs = [np.empty((64, 64, 2), np.float32), np.empty((64, 64, 2), np.int32), np.empty((64, 64, 2), np.int32), np.empty((64, 64), np.uint8), np.empty(12, np.int32)]
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(ctx.h).decode()
    call = lambda i0=P(a), i1=P(b), cn=1, order=0, stride=64, w=64, h=64, L=2, iters=6, shift=1024, eig=0, alpha=10, beta=32768, o=tuple(P(x) for x in outs), dev=0: f(
        ctx.h, i0, i1, cn, order, stride, w, h, L, iters, shift, eig, alpha, beta, *o, dev)
    assert call() == 0
    assert call(i0=None) == -1 and "image" in err()
    assert call(i1=None) == -1 and "image" in err()
    for w, h in ((15, 64), (64, 15), (4096, 64), (64, 4096), (0, 0), (-1, 64)):
        assert call(w=w, h=h, stride=max(w, 64)) == -1 and "size" in err()
    for cn in (0, 2, 5, -1):
        assert call(cn=cn, stride=64 * 8) == -1 and "channels" in err()
    assert call(stride=63) == -1 and "stride" in err()
    for L in (-1, 7, 4):
        assert call(L=L) == -1 and "coarsest" in err()
    for iters in (0, 17):
        assert call(iters=iters) == -1 and "iters" in err()
    for shift in (-1, 2049):
        assert call(shift=shift) == -1 and "max_shift_q8" in err()
    assert call(eig=-1) == -1 and "min_eig" in err()
    for alpha in (-1, 1025):
        assert call(alpha=alpha) == -1 and "alpha_q10" in err()
    for beta in (-1, (1 << 30) + 1):
        assert call(beta=beta) == -1 and "beta_q16" in err()
    assert call(o=(None,) * 5) == -1 and "output" in err()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    t = [torch.zeros(64 * 64 * 2 + 2, dtype=torch.int32, device="cuda") for _ in range(5)]
    dp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    for k, off in ((0, 4), (1, 4), (2, 4), (4, 2)):                                           # device form, one misaligned output: refused before any launch
        o = tuple(dp(t[i], off if i == k else 0) for i in range(5))
        assert call(i0=dp(ta), i1=dp(tb), o=o, dev=1) == -1 and "aligned" in err()
    assert f(None, P(a), P(b), 1, 0, 64, 64, 64, 2, 6, 1024, 0, 10, 32768, *[P(x) for x in outs], 0) == -1
    with pytest.raises(vido.VidoError):
        ctx.dis_flow_pair(a, b[:32])
    _same(ctx.dis_flow_pair(a, b, coarsest=2), good)


def test_hipops_form_on_torch_tensors(vido, ctx):
    """HipOps.dis_flow_pair on u8 device tensors, grey and BGR, on torch's current stream: equal to the host form; dis_flow's argument checks."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    a, b = _occluded(vido, 73, 50, seed=51)
    ca, cb = np.ascontiguousarray(np.stack([a, np.roll(a, 1, 1), 255 - a], -1)), np.ascontiguousarray(np.stack([b, np.roll(b, 1, 1), 255 - b], -1))
    for i0, i1 in ((a, b), (ca, cb)):
        want = ctx.dis_flow_pair(i0, i1, coarsest=2, iters=4, beta_q16=8192)
        t0, t1 = torch.from_numpy(i0).cuda(), torch.from_numpy(i1).cuda()
        fwd = torch.full((50, 73, 2), -77, dtype=torch.int32, device="cuda"); bwd = fwd.clone()
        status = torch.full((50, 73), 77, dtype=torch.uint8, device="cuda"); stats = torch.full((12,), -77, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            flow = ops.dis_flow_pair(t0, t1, fwd_q8=fwd, bwd_q8=bwd, status=status, stats=stats, coarsest=2, iters=4, beta_q16=8192)
        side.synchronize()
        _same(tuple(x.cpu().numpy() for x in (flow, fwd, bwd, status, stats)), want)
        out = torch.empty((50, 73, 2), dtype=torch.float32, device="cuda")
        assert ops.dis_flow_pair(t0, t1, out=out, coarsest=2, iters=4, beta_q16=8192) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    t0, t1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    bad = [(t0.cpu(), t1, {}), (t0, t1.float(), {}), (t0, t1[:, :64].contiguous(), {}), (t0[:, ::2], t1[:, ::2], {}), (t0[None], t1[None], {}),
           (torch.from_numpy(np.stack([a, a], -1)).cuda(), torch.from_numpy(np.stack([b, b], -1)).cuda(), {}),
           (t0, t1, dict(out=torch.empty((50, 73), dtype=torch.float32, device="cuda"))), (t0, t1, dict(out=torch.empty((50, 73, 2), dtype=torch.float64, device="cuda"))),
           (t0, t1, dict(fwd_q8=torch.empty((50, 73, 2), dtype=torch.int64, device="cuda"))), (t0, t1, dict(bwd_q8=torch.empty((50, 72, 2), dtype=torch.int32, device="cuda"))),
           (t0, t1, dict(status=torch.empty((50, 73), dtype=torch.int32, device="cuda"))), (t0, t1, dict(stats=torch.empty((11,), dtype=torch.int32, device="cuda"))),
           (t0, t1, dict(out=torch.empty((50, 73, 2), dtype=torch.float32))), (t0, t1, dict(iters=17)), (t0, t1, dict(beta_q16=-1))]
    for x, y, kw in bad:
        with pytest.raises(vido.VidoError):
            ops.dis_flow_pair(x, y, **kw)
    _same(ctx.dis_flow_pair(a, b, coarsest=2), _statement(a, b, coarsest=2))
