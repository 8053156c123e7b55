"""MI355X: vido_flow_consistency (csrc/flowcheck.hip: k_flow_check) against the numpy statement (tests/refimpl/flow_consistency_np.py): status, marked flow (compared as
uint32) and stats bit for bit, no tolerance anywhere.  Inputs: the constructed fields of tests/refimpl/flow_consistency_cases.py (5 x 4, 16 x 16, 4095 x 1), random fields
at 16 x 16, 73 x 50 and 201 x 151 with magnitudes up to 2^19 - 1 and a sprinkling at +-2^19, H = 1 and W = 1; the host and the device form, each output NULL in turn, sizes in
turn on one context, every refusal, the HipOps form.  The context is configured for 64 x 64: the op does not depend on that."""
import ctypes as C
import numpy as np
import pytest

from refimpl import flow_consistency_np as F
from refimpl import flow_consistency_cases as K

pytestmark = pytest.mark.gpu

NAMES = ("status", "marked", "stats")


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _same(got, want):
    assert len(got) == len(want) == 3
    for g, w_, name in zip(got, want, NAMES):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if g.dtype == np.float32:
            g, w_ = g.view(np.uint32), w_.view(np.uint32)                                     # NaNs compare by their bits
        if not np.array_equal(g, w_):
            bad = np.argwhere(g != w_)
            assert False, (name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])


@pytest.mark.parametrize("case", K.constructed(), ids=lambda c: c[0])
def test_bit_equal_on_the_constructed_fields(ctx, case):
    name, fwd, bwd, alpha, beta = case
    want = F.flow_consistency(fwd, bwd, alpha, beta)
    print("%-24s stats %s" % (name, want[2].tolist()))
    _same(ctx.flow_consistency(fwd, bwd, alpha, beta), want)


@pytest.mark.parametrize("w,h", [(16, 16), (73, 50), (201, 151), (1, 1), (1, 37), (300, 1)])
def test_bit_equal_on_random_fields(ctx, w, h):
    fwd, bwd = K.random_fields(h, w, seed=w + h)
    if h == 1:
        fwd[..., 1] = 0                                                                       # (a single row or column: any motion across it leaves the image)
    if w == 1:
        fwd[..., 0] = 0
    seen = np.zeros(4, np.int64)
    for alpha, beta in ((10, 32768), (0, 0), (1024, 1 << 30), (1024, 0), (3, 1 << 20)):
        want = F.flow_consistency(fwd, bwd, alpha, beta)
        seen += want[2]
        _same(ctx.flow_consistency(fwd, bwd, alpha, beta), want)
    print("%d x %d: statuses seen over five parameter pairs %s" % (w, h, seen.tolist()))
    if w * h > 200:
        assert (seen > 0).all()                                                               # every status occurs, the limit's sprinkling included


def test_device_form_equals_host_form_with_and_without_each_output(ctx):
    import torch
    fwd, bwd = K.random_fields(50, 73, seed=9)
    want = ctx.flow_consistency(fwd, bwd)
    _same(want, F.flow_consistency(fwd, bwd))
    tf, tb = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    shapes = ((50, 73), (50, 73, 2), (4,)); dtypes = (torch.uint8, torch.float32, torch.int32)
    for mask in (1, 2, 4, 3, 5, 6, 7):
        outs = [torch.full(s, 77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
        torch.cuda.synchronize()
        ptrs = [o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)]
        ctx.flow_consistency_device(tf.data_ptr(), tb.data_ptr(), 50, 73, status_ptr=ptrs[0], marked_ptr=ptrs[1], stats_ptr=ptrs[2])
        ctx.synchronize()
        for i, o in enumerate(outs):
            if mask >> i & 1:
                got = o.cpu().numpy()
                assert np.array_equal(got.view(np.uint32) if i == 1 else got, want[i].view(np.uint32) if i == 1 else want[i]), (mask, i)
            else:
                assert bool((o == 77).all()), (mask, i)
    lib = ctx.lib                                                                             # the host form without each output
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    for mask in (1, 2, 4):
        outs = [np.full((50, 73), 77, np.uint8), np.full((50, 73, 2), 77, np.float32), np.full(4, 77, np.int32)]
        assert lib.vido_flow_consistency(ctx.h, P(fwd), P(bwd), 50, 73, 10, 32768, *[P(o) if mask >> i & 1 else None for i, o in enumerate(outs)], 0) == 0
        for i, o in enumerate(outs):
            assert np.array_equal(o.view(np.uint32) if i == 1 else o, want[i].view(np.uint32) if i == 1 else want[i]) if mask >> i & 1 else (o == 77).all(), (mask, i)


def test_sizes_in_turn_on_one_context(ctx):
    a = K.random_fields(64, 64, seed=31); b = K.random_fields(151, 201, seed=32); c = K.random_fields(4, 5, seed=33)
    first = ctx.flow_consistency(*a)
    _same(first, F.flow_consistency(*a))
    _same(ctx.flow_consistency(*b), F.flow_consistency(*b))
    _same(ctx.flow_consistency(*c), F.flow_consistency(*c))
    _same(ctx.flow_consistency(*a), first)


def test_every_refusal_leaves_the_context_usable(vido, ctx):
    import torch
    fwd, bwd = K.random_fields(16, 16, seed=41)
    good = ctx.flow_consistency(fwd, bwd)
    lib = ctx.lib; f = lib.vido_flow_consistency
    status = np.empty((16, 16), np.uint8); marked = np.empty((16, 16, 2), np.float32); stats = np.empty(4, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(ctx.h).decode()
    call = lambda a=P(fwd), b=P(bwd), h=16, w=16, alpha=10, beta=32768, o=(P(status), P(marked), P(stats)), dev=0: f(ctx.h, a, b, h, w, alpha, beta, *o, dev)
    assert call() == 0
    assert call(a=None) == -1 and "field" in err()
    assert call(b=None) == -1 and "field" in err()
    for h, w in ((0, 16), (16, 0), (4096, 16), (16, 4096), (-1, 16), (0, 0)):
        assert call(h=h, w=w) == -1 and "size" in err()
    for alpha in (-1, 1025, 1 << 20):
        assert call(alpha=alpha) == -1 and "alpha_q10" in err()
    for beta in (-1, (1 << 30) + 1, -(1 << 31)):
        assert call(beta=beta) == -1 and "beta_q16" in err()
    assert call(alpha=1024, beta=1 << 30) == 0 and call(alpha=0, beta=0) == 0
    assert call(o=(None, None, None)) == -1 and "output" in err()
    tf, tb = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    t = [torch.zeros(16 * 16 * 2 + 2, dtype=torch.int32, device="cuda") for _ in range(3)]
    dp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    assert call(a=dp(tf), b=dp(tb), o=(dp(t[0]), dp(t[1]), dp(t[2])), dev=1) == 0
    for o in ((dp(t[0]), dp(t[1], 4), dp(t[2])), (dp(t[0]), dp(t[1]), dp(t[2], 2))):           # device form, a misaligned output: refused before any launch
        assert call(a=dp(tf), b=dp(tb), o=o, dev=1) == -1 and "aligned" in err()
    assert call(a=dp(t[0], 4), b=dp(tb), o=(dp(t[0]), dp(t[1]), dp(t[2])), dev=1) == -1 and "aligned" in err()
    ctx.synchronize()
    assert f(None, P(fwd), P(bwd), 16, 16, 10, 32768, P(status), P(marked), P(stats), 0) == -1
    for a, b in ((fwd, bwd[:8]), (fwd.astype(np.int64), bwd), (fwd[..., 0], bwd[..., 0])):
        with pytest.raises(vido.VidoError):
            ctx.flow_consistency(a, b)
    _same(ctx.flow_consistency(fwd, bwd), good)


def test_hipops_form_on_torch_tensors(vido, ctx):
    """HipOps.flow_consistency on device tensors, on torch's current stream: equal to the host form; wrong device, dtype, shape or contiguity raises."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    fwd, bwd = K.random_fields(50, 73, seed=51)
    want = ctx.flow_consistency(fwd, bwd, alpha_q10=20, beta_q16=8192)
    tf, tb = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    status = torch.full((50, 73), 77, dtype=torch.uint8, device="cuda"); stats = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        marked = ops.flow_consistency(tf, tb, status=status, stats=stats, alpha_q10=20, beta_q16=8192)
    side.synchronize()
    _same((status.cpu().numpy(), marked.cpu().numpy(), stats.cpu().numpy()), want)
    out = torch.empty((50, 73, 2), dtype=torch.float32, device="cuda")
    assert ops.flow_consistency(tf, tb, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), F.flow_consistency(fwd, bwd)[1].view(np.uint32))      # the defaults are the statement's
    bad = [(tf.cpu(), tb, {}), (tf, tb.float(), {}), (tf, tb[:, :64].contiguous(), {}), (tf[:, ::2], tb[:, ::2], {}), (tf[..., 0], tb[..., 0], {}),
           (tf, tb, dict(out=torch.empty((50, 73), dtype=torch.float32, device="cuda"))), (tf, tb, dict(out=torch.empty((50, 73, 2), dtype=torch.float64, device="cuda"))),
           (tf, tb, dict(status=torch.empty((50, 73), dtype=torch.int32, device="cuda"))), (tf, tb, dict(status=torch.empty((50, 72), dtype=torch.uint8, device="cuda"))),
           (tf, tb, dict(stats=torch.empty((3,), dtype=torch.int32, device="cuda"))), (tf, tb, dict(out=torch.empty((50, 73, 2), dtype=torch.float32))), (tf, tb, dict(alpha_q10=1025))]
    for x, y, kw in bad:
        with pytest.raises(vido.VidoError):
            ops.flow_consistency(x, y, **kw)
    _same(ctx.flow_consistency(fwd, bwd), F.flow_consistency(fwd, bwd))
