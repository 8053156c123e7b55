"""MI355X: vido_stereo_sgm (csrc/stereosgm.hip: k_sgm_ingest, k_sgm_census, k_sgm_path, k_sgm_select) against the numpy statement (tests/refimpl/stereo_sgm_np.py):
disp, q4, status and stats bit for bit, no tolerance anywhere.  Shapes (w, h, D): 16 x 16 x 16 (four lines per wave), 17 x 16 x 64 (width below D: most of C is the constant
64), 64 x 48 x 64 (one lane per disparity), 73 x 50 x 48 (odd sizes, idle lanes), 201 x 151 x 128 (two per lane, more than one selection step per wave), 130 x 20 x 256
(four per lane); hostile content at 96 x 32 x 32 (two lines per wave); parameter edges; strides, channels, the host and the device form, sizes in turn on one context,
every refusal, the HipOps form and a captured graph.  The context is configured for 64 x 64: the op does not depend on that.  Each GPU step runs under limit()."""
import ctypes as C
import numpy as np
import pytest

from refimpl import stereo_sgm_np as G
from refimpl import stereo_cases as K
from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

NAMES = ("disp", "q4", "status", "stats")
SHAPES = [(16, 16, 16), (17, 16, 64), (64, 48, 64), (73, 50, 48), (201, 151, 128), (130, 20, 256)]


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w_, name in zip(got, want, NAMES):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if not np.array_equal(g, w_):
            bad = np.argwhere(g != w_)
            assert False, (name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])
    ok = got[2] == 0
    assert np.array_equal(got[0][ok], got[1][ok].astype(np.float32) / np.float32(16)) and (got[0][~ok] == -1).all()      # disp == q4 / 16 exactly where valid, -1 elsewhere


@pytest.mark.parametrize("w,h,D", SHAPES)
def test_bit_equal_at_the_small_shapes(ctx, w, h, D):
    left, right = K.warped_pair(w, h, D, seed=w + D)
    want, S, Cv = K.run(left, right, max_disp=D)
    d0 = S.argmin(2)
    print("stereo_sgm %d x %d x %d: stats %s, d0 %d..%d, share of C at 64: %.2f, pixels with a tie in S: %d" % (
        w, h, D, want[3].tolist(), d0.min(), d0.max(), (Cv == 64).mean(), ((S == S.min(2, keepdims=True)).sum(2) > 1).sum()))
    assert (want[3][:3] > 0).all() and d0.min() == 0 and d0.max() >= min(D, w) // 5
    if (w, D) == (17, 64):
        assert (Cv == 64).mean() > 0.8
    if D == 128:
        assert d0.max() == D - 1                                                            # both lane-edge disparities win somewhere
    with limit(60, "vido_stereo_sgm %d x %d x %d" % (w, h, D)):
        got = ctx.stereo_sgm(left, right, max_disp=D)
    _same(got, want)


def test_hostile_content(ctx):
    seen = np.zeros(4, np.int64)
    for name, left, right, kw, shows in K.hostile_cases(96, 32, 32):
        want, S, Cv = K.run(left, right, max_disp=32, **kw)
        print("%-40s stats %s" % (name, want[3].tolist()))
        assert shows(want, S, Cv), name
        seen += want[3]
        with limit(60, name):
            got = ctx.stereo_sgm(left, right, max_disp=32, **kw)
        _same(got, want)
    assert (seen > 0).all()


def test_parameter_edges(ctx):
    left, right = K.warped_pair(73, 50, 48, seed=7)
    base = K.run(left, right, max_disp=48)[0]
    for kw in (dict(p1=0, p2=0), dict(p1=1000, p2=1000), dict(p1=0, p2=1000), dict(uniqueness=0), dict(uniqueness=99), dict(lr_tol=0), dict(lr_tol=255)):
        want = K.run(left, right, max_disp=48, **kw)[0]
        print("%-28s stats %s" % (kw, want[3].tolist()))
        assert not np.array_equal(want[2], base[2]), kw                                      # the parameter matters on this pair
        with limit(60, str(kw)):
            got = ctx.stereo_sgm(left, right, max_disp=48, **kw)
        _same(got, want)
    assert K.run(left, right, max_disp=48, uniqueness=99)[0][3][1] > base[3][1] and K.run(left, right, max_disp=48, lr_tol=255)[0][3][2] < base[3][2]


def test_row_stride_and_channels(ctx):
    rng = np.random.RandomState(4)
    left, right = K.warped_pair(73, 50, 48, seed=5)
    want = G.stereo_sgm(left, right, max_disp=48)
    wide = [np.full((50, 96), 7, np.uint8) for _ in range(2)]
    wide[0][:, :73] = left; wide[1][:, :73] = right
    with limit(120, "strides and channels"):
        _same(ctx.stereo_sgm(wide[0][:, :73], wide[1][:, :73], max_disp=48), want)              # stride 96 > width 73
        for cn in (3, 4):
            c0 = rng.randint(0, 256, (50, 73 + 48, cn)).astype(np.uint8)
            c1 = np.ascontiguousarray(c0[:, 9:9 + 73]); c0 = np.ascontiguousarray(c0[:, :73])      # the right view shows the left's column x + 9, channels that differ
            for order in (0, 1):
                w_ = G.stereo_sgm(c0, c1, max_disp=48, rgb_order=order)
                _same(ctx.stereo_sgm(c0, c1, max_disp=48, rgb_order=order), w_)
                _same(ctx.stereo_sgm(G.grey(c0, order).astype(np.uint8), G.grey(c1, order).astype(np.uint8), max_disp=48), w_)
            assert not np.array_equal(G.stereo_sgm(c0, c1, max_disp=48, rgb_order=0)[1], G.stereo_sgm(c0, c1, max_disp=48, rgb_order=1)[1])
            pad = [np.zeros((50, 73 * cn + 11), np.uint8) for _ in range(2)]                    # a colour row stride that is no multiple of the pixel
            pad[0][:, :73 * cn] = c0.reshape(50, -1); pad[1][:, :73 * cn] = c1.reshape(50, -1)
            v0 = np.lib.stride_tricks.as_strided(pad[0], (50, 73, cn), (pad[0].strides[0], cn, 1)); v1 = np.lib.stride_tricks.as_strided(pad[1], (50, 73, cn), (pad[1].strides[0], cn, 1))
            _same(ctx.stereo_sgm(v0, v1, max_disp=48, rgb_order=1), G.stereo_sgm(c0, c1, max_disp=48, rgb_order=1))


def test_device_form_equals_host_form_with_and_without_each_output(ctx):
    import torch
    left, right = K.warped_pair(73, 50, 48, seed=9)
    with limit(120, "device form, every subset of the outputs"):
        want = ctx.stereo_sgm(left, right, max_disp=48)
        _same(want, G.stereo_sgm(left, right, max_disp=48))
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        shapes = ((50, 73), (50, 73), (50, 73), (4,)); dtypes = (torch.float32, torch.int32, torch.uint8, torch.int32)
        for mask in range(1, 16):
            outs = [torch.full(s, 77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
            torch.cuda.synchronize()
            ptrs = [o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)]
            ctx.stereo_sgm_device(tl.data_ptr(), tr.data_ptr(), 1, 73, 73, 50, max_disp=48, disp_ptr=ptrs[0], q4_ptr=ptrs[1], status_ptr=ptrs[2], stats_ptr=ptrs[3])
            ctx.synchronize()
            for i, o in enumerate(outs):
                assert np.array_equal(o.cpu().numpy(), want[i]) if mask >> i & 1 else bool((o == 77).all()), (mask, i)


def test_sizes_in_turn_on_one_context(ctx):
    a = K.warped_pair(64, 48, 64, seed=31); b = K.warped_pair(201, 151, 128, seed=32); c = K.warped_pair(16, 16, 16, seed=33)
    with limit(120, "grow, shrink, grow"):
        first = ctx.stereo_sgm(*a, max_disp=64)
        _same(first, G.stereo_sgm(*a, max_disp=64))
        _same(ctx.stereo_sgm(*b, max_disp=128), G.stereo_sgm(*b, max_disp=128))
        _same(ctx.stereo_sgm(*c, max_disp=16), G.stereo_sgm(*c, max_disp=16))
        _same(ctx.stereo_sgm(*a, max_disp=64), first)
        _same(ctx.stereo_sgm(*a, max_disp=32), G.stereo_sgm(*a, max_disp=32))
        _same(ctx.stereo_sgm(*b, max_disp=256), G.stereo_sgm(*b, max_disp=256))
        _same(ctx.stereo_sgm(*a, max_disp=64), first)


def test_every_refusal_leaves_the_context_usable(vido, ctx):
    import torch
    left, right = K.warped_pair(64, 64, 32, seed=41)
    with limit(120, "refusals"):
        good = ctx.stereo_sgm(left, right, max_disp=32)
        lib = ctx.lib; f = lib.vido_stereo_sgm
        disp = np.empty((64, 64), np.float32); q4 = np.empty((64, 64), np.int32); status = np.empty((64, 64), np.uint8); stats = np.empty(4, np.int32)
        P = lambda x: x.ctypes.data_as(C.c_void_p)
        err = lambda: lib.vido_last_error(ctx.h).decode()
        call = lambda i0=P(left), i1=P(right), cn=1, order=0, stride=64, w=64, h=64, D=32, p1=10, p2=120, u=10, lr=1, o=(P(disp), P(q4), P(status), P(stats)), dev=0: f(
            ctx.h, i0, i1, cn, order, stride, w, h, D, p1, p2, u, lr, *o, dev)
        assert call() == 0
        assert call(i0=None) == -1 and "image" in err()
        assert call(i1=None) == -1 and "image" in err()
        for w, h in ((15, 64), (64, 15), (4096, 64), (64, 4096), (0, 0), (-1, 64)):
            assert call(w=w, h=h, stride=max(w, 64)) == -1 and "size" in err()
        for cn in (0, 2, 5, -1):
            assert call(cn=cn, stride=64 * 8) == -1 and "channels" in err()
        assert call(stride=63) == -1 and "stride" in err()
        assert call(cn=3, stride=191) == -1 and "stride" in err()
        for D in (0, 8, 24, 100, 272, -16, 1 << 20):
            assert call(D=D) == -1 and "max_disp" in err()
        assert call(w=2048, h=2048, stride=2048, D=128) == -1 and "volume" in err()                # 2^29 cells: refused before anything is read
        for p1, p2 in ((-1, 120), (121, 120), (10, 1001), (1001, 1001)):
            assert call(p1=p1, p2=p2) == -1 and "penalties" in err()
        for u in (-1, 100):
            assert call(u=u) == -1 and "uniqueness" in err()
        for lr in (-1, 256):
            assert call(lr=lr) == -1 and "lr_tol" in err()
        assert call(o=(None, None, None, None)) == -1 and "output" in err()
        tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        t = [torch.zeros(64 * 64 + 1, dtype=torch.int32, device="cuda") for _ in range(4)]
        dp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
        for k in (0, 1, 3):                                                                     # device form, one misaligned 4-byte output: refused before any launch
            o = tuple(dp(t[i], 2 if i == k else 0) for i in range(4))
            assert call(i0=dp(tl), i1=dp(tr), o=o, dev=1) == -1 and "aligned" in err()
        assert f(None, P(left), P(right), 1, 0, 64, 64, 64, 32, 10, 120, 10, 1, P(disp), P(q4), P(status), P(stats), 0) == -1
        with pytest.raises(vido.VidoError):
            ctx.stereo_sgm(left, right[:32])
        with pytest.raises(vido.VidoError):
            ctx.stereo_sgm(left, right, max_disp=40)
        _same(ctx.stereo_sgm(left, right, max_disp=32), good)
    _same(good, G.stereo_sgm(left, right, max_disp=32))


def test_hipops_form_on_torch_tensors(vido, ctx):
    """HipOps.stereo_sgm on u8 device tensors, grey and BGR, on torch's current stream: equal to the host form; wrong device, dtype, shape or contiguity raises."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    a, b = K.warped_pair(73, 50, 48, seed=51)
    ca, cb = np.ascontiguousarray(np.stack([a, np.roll(a, 1, 0), 255 - a], -1)), np.ascontiguousarray(np.stack([b, np.roll(b, 1, 0), 255 - b], -1))
    with limit(120, "HipOps.stereo_sgm"):
        for i0, i1 in ((a, b), (ca, cb)):
            want = ctx.stereo_sgm(i0, i1, max_disp=48, p2=90)
            t0, t1 = torch.from_numpy(i0).cuda(), torch.from_numpy(i1).cuda()
            q4 = torch.full((50, 73), -77, dtype=torch.int32, device="cuda"); status = torch.full((50, 73), 77, dtype=torch.uint8, device="cuda")
            stats = torch.full((4,), -77, dtype=torch.int32, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                disp = ops.stereo_sgm(t0, t1, q4=q4, status=status, stats=stats, max_disp=48, p2=90)
            side.synchronize()
            _same((disp.cpu().numpy(), q4.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()), want)
            out = torch.empty((50, 73), dtype=torch.float32, device="cuda")
            assert ops.stereo_sgm(t0, t1, out=out, max_disp=48, p2=90) is out
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want[0])
        _same(ctx.stereo_sgm(a, b, max_disp=48, p2=90), G.stereo_sgm(a, b, max_disp=48, p2=90))
        t0, t1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        bad = [(t0.cpu(), t1, {}), (t0, t1.float(), {}), (t0, t1[:, :64].contiguous(), {}), (t0[:, ::2], t1[:, ::2], {}), (t0[None], t1[None], {}),
               (torch.from_numpy(np.stack([a, a], -1)).cuda(), torch.from_numpy(np.stack([b, b], -1)).cuda(), {}),
               (t0, t1, dict(out=torch.empty((50, 73, 1), dtype=torch.float32, device="cuda"))), (t0, t1, dict(out=torch.empty((50, 73), dtype=torch.float64, device="cuda"))),
               (t0, t1, dict(q4=torch.empty((50, 73), dtype=torch.int64, device="cuda"))), (t0, t1, dict(status=torch.empty((50, 73), dtype=torch.int32, device="cuda"))),
               (t0, t1, dict(stats=torch.empty((3,), dtype=torch.int32, device="cuda"))), (t0, t1, dict(out=torch.empty((50, 73), dtype=torch.float32))),
               (t0, t1, dict(max_disp=40))]
        for x, y, kw in bad:
            with pytest.raises(vido.VidoError):
                ops.stereo_sgm(x, y, **{**dict(max_disp=48), **kw})
        _same(ctx.stereo_sgm(a, b, max_disp=48), G.stereo_sgm(a, b, max_disp=48))


def test_captured_graph_replayed_on_new_contents(vido, ctx):
    """The device form inside torch.cuda.graph (after one eager call of the size, which grows the scratch): a replay on new image contents equals the eager call on them."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    a = K.warped_pair(73, 50, 48, seed=61); b = K.warped_pair(73, 50, 48, seed=62)
    want_a, want_b = G.stereo_sgm(*a, max_disp=48), G.stereo_sgm(*b, max_disp=48)
    assert not np.array_equal(want_a[1], want_b[1])
    with limit(120, "capture and two replays"):
        tl, tr = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
        outs = [torch.zeros((50, 73), dtype=torch.float32, device="cuda"), torch.zeros((50, 73), dtype=torch.int32, device="cuda"),
                torch.zeros((50, 73), dtype=torch.uint8, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda")]
        run = lambda: ops.stereo_sgm(tl, tr, out=outs[0], q4=outs[1], status=outs[2], stats=outs[3], max_disp=48)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side); torch.cuda.synchronize()
        _same(tuple(o.cpu().numpy() for o in outs), want_a)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        torch.cuda.synchronize()
        for pair, want in ((b, want_b), (a, want_a)):
            tl.copy_(torch.from_numpy(pair[0])); tr.copy_(torch.from_numpy(pair[1]))
            for o in outs:
                o.fill_(5)
            g.replay()
            torch.cuda.synchronize()
            _same(tuple(o.cpu().numpy() for o in outs), want)
