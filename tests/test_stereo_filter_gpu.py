"""MI355X: vido_stereo_filter (csrc/stereofilter.hip: k_sf_local, k_sf_seam, k_sf_flatten, k_sf_write) against the numpy statement (tests/refimpl/stereo_filter_np.py):
disp, status, depth and stats bit for bit, no tolerance anywhere.  Inputs: every case of tests/refimpl/stereo_filter_cases.py — random q4 / status on 1 x 1, 1 x 67,
67 x 1, 31 x 33, 33 x 31, 97 x 130, 64 x 64 and 32 x 32 (exactly one tile), every cc_patterns geometry as the validity mask, the ramps that are one region only because the
relation is not transitive, and the SGM statement's own output; parameter edges; status_out aliasing status, every subset of NULL outputs, the host and the device form,
a captured graph replayed on other contents, two sizes in turn, HipOps on a side stream and every refusal.  The context is configured for 64 x 64: the op does not
depend on that.  Each GPU step runs under limit()."""
import ctypes as C
import numpy as np
import pytest

from refimpl import stereo_filter_np as F
from refimpl import stereo_filter_cases as CASES
from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

NAMES = ("disp", "status", "depth", "stats")
ALL = CASES.all_cases()


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _want(q4, status, **kw):
    with np.errstate(over="ignore"):
        return F.stereo_filter(q4, status, **kw)


def _same(got, want):
    assert len(got) == len(want) == 4
    for g, w_, name in zip(got, want, NAMES):
        if w_ is None:
            assert g is None, name
            continue
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if g.tobytes() != w_.tobytes():
            gb, wb = g.view(np.uint32 if g.itemsize == 4 else np.uint8), w_.view(np.uint32 if g.itemsize == 4 else np.uint8)
            bad = np.argwhere(gb != wb)
            assert False, (name, len(bad), bad[:6].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])


@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_bit_equal_on_every_case(ctx, case):
    name, q4, status, params, shows = case
    assert shows(F), "the case is not what its name says"
    want = _want(q4, status, bf=75.0, **params)
    print("%-28s %s: stats %s" % (name, params, want[3].tolist()))
    with limit(60, name):
        got = ctx.stereo_filter(q4, status, bf=75.0, **params)
    _same(got, want)


def test_parameter_edges(ctx):
    name, q4, status, params, _ = ALL[5]                                                      # random 97 x 130
    assert q4.shape == (97, 130)
    area = F.region_areas(q4, status, 8)[1]
    a = int(area.max())
    seen = set()
    with limit(120, "parameter edges"):
        for kw in (dict(max_diff_q4=8, min_region=1), dict(max_diff_q4=8, min_region=a), dict(max_diff_q4=8, min_region=a + 1), dict(max_diff_q4=8, min_region=1 << 24),
                   dict(max_diff_q4=0, min_region=2), dict(max_diff_q4=65535, min_region=97 * 130), dict(max_diff_q4=65535, min_region=2)):
            want = _want(q4, status, bf=0.1, **kw)
            print("%-46s stats %s" % (kw, want[3].tolist()))
            seen.add(tuple(want[3].tolist()))
            _same(ctx.stereo_filter(q4, status, bf=0.1, **kw), want)
        assert len(seen) >= 6                                                                  # the edges matter on this input
        assert _want(q4, status, max_diff_q4=8, min_region=a)[3][3] > 0 and _want(q4, status, max_diff_q4=8, min_region=a + 1)[3][3] == 0
        # statuses copied through, bad disparities marked, the depth's bits: the statement's small inputs
        q = np.array([[48, 48, 48, 48, 48, 0, -5, 65536, 65535, 1, 3, 7]], np.int32); s = np.array([[0, 1, 2, 3, 200, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
        for bf in (75.0, 0.1, 1e-38, 3e38, 250.0):
            for m in (1, 2, 4):
                want = _want(q, s, max_diff_q4=65535, min_region=m, bf=bf)
                assert (want[2].view(np.uint32)[want[1] != 0] == 0x7F7FFFFF).all()
                _same(ctx.stereo_filter(q, s, max_diff_q4=65535, min_region=m, bf=bf), want)
        assert ctx.stereo_filter(q, s, max_diff_q4=65535, min_region=1)[2] is None


def test_device_form_status_in_place_and_every_subset_of_outputs(ctx):
    import torch
    name, q4, status, params, _ = ALL[5]
    h, w = q4.shape
    want = _want(q4, status, bf=12.5, **params)
    with limit(120, "device form, every subset of the outputs"):
        _same(ctx.stereo_filter(q4, status, bf=12.5, **params), want)
        tq = torch.from_numpy(q4).cuda()
        shapes = ((h, w), (h, w), (h, w), (4,)); dtypes = (torch.float32, torch.uint8, torch.float32, torch.int32)
        for mask in range(1, 16):
            outs = [torch.full(s, 77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
            ts = torch.from_numpy(status).cuda()
            torch.cuda.synchronize()
            ptrs = [o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)]
            ctx.stereo_filter_device(tq.data_ptr(), ts.data_ptr(), w, h, bf=12.5, disp_ptr=ptrs[0], status_out_ptr=ptrs[1], depth_ptr=ptrs[2], stats_ptr=ptrs[3], **params)
            ctx.synchronize()
            for i, o in enumerate(outs):
                assert o.cpu().numpy().tobytes() == want[i].tobytes() if mask >> i & 1 else bool((o == 77).all()), (mask, i)
            assert np.array_equal(ts.cpu().numpy(), status)
            if mask & 2:                                                                        # the same call with status_out BEING status
                for o in outs:
                    o.fill_(77)
                ptrs[1] = ts.data_ptr()
                ctx.stereo_filter_device(tq.data_ptr(), ts.data_ptr(), w, h, bf=12.5, disp_ptr=ptrs[0], status_out_ptr=ptrs[1], depth_ptr=ptrs[2], stats_ptr=ptrs[3], **params)
                ctx.synchronize()
                assert np.array_equal(ts.cpu().numpy(), want[1])
                for i in (0, 2, 3):
                    o = outs[i]
                    assert o.cpu().numpy().tobytes() == want[i].tobytes() if mask >> i & 1 else bool((o == 77).all()), (mask, i, "in place")
        # the op on its own output: nothing is valid that was not, nothing is removed twice at the same parameters unless a region shrank below the bar — equal to the statement
        again = _want(q4, want[1], bf=12.5, **params)
        _same(ctx.stereo_filter(q4, want[1], bf=12.5, **params), again)


def test_two_sizes_in_turn_on_one_context(ctx):
    a, b = ALL[5], ALL[1]                                                                      # 97 x 130, 1 x 67
    big = CASES.random_case(150, 201, 77)
    with limit(120, "grow, shrink, grow"):
        first = ctx.stereo_filter(a[1], a[2], bf=75.0, **a[3])
        _same(first, _want(a[1], a[2], bf=75.0, **a[3]))
        for _ in range(2):
            _same(ctx.stereo_filter(b[1], b[2], bf=75.0, **b[3]), _want(b[1], b[2], bf=75.0, **b[3]))
            _same(ctx.stereo_filter(big[0], big[1], max_diff_q4=8, min_region=6), _want(big[0], big[1], max_diff_q4=8, min_region=6))
            _same(ctx.stereo_filter(a[1], a[2], bf=75.0, **a[3]), first)


def test_hipops_form_on_a_side_stream(vido, ctx):
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    name, q4, status, params, _ = ALL[5]
    h, w = q4.shape
    want = _want(q4, status, bf=75.0, **params)
    with limit(120, "HipOps.stereo_filter"):
        tq, ts = torch.from_numpy(q4).cuda(), torch.from_numpy(status).cuda()
        st = torch.full((h, w), 77, dtype=torch.uint8, device="cuda"); depth = torch.full((h, w), 77.0, dtype=torch.float32, device="cuda")
        stats = torch.full((4,), -77, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            disp = ops.stereo_filter(tq, ts, status_out=st, depth=depth, stats=stats, bf=75.0, **params)
        side.synchronize()
        _same((disp.cpu().numpy(), st.cpu().numpy(), depth.cpu().numpy(), stats.cpu().numpy()), want)
        out = torch.empty((h, w), dtype=torch.float32, device="cuda")
        assert ops.stereo_filter(tq, ts, out=out, status_out=ts, **params) is out              # in place, no depth, no stats
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(ts.cpu().numpy(), want[1])
        ts = torch.from_numpy(status).cuda()
        dflt = ops.stereo_filter(tq, ts)                                                       # the defaults are the statement's
        torch.cuda.synchronize()
        assert np.array_equal(dflt.cpu().numpy(), _want(q4, status)[0])
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        bad = [(tq.cpu(), ts, {}), (tq, ts.cpu(), {}), (tq.float(), ts, {}), (tq, ts.int(), {}), (tq, ts[:, :64].contiguous(), {}), (tq[:, ::2], ts[:, ::2], {}), (tq[None], ts[None], {}),
               (tq, ts, dict(out=f32(h, w, 1))), (tq, ts, dict(out=torch.empty((h, w), dtype=torch.float64, device="cuda"))), (tq, ts, dict(out=torch.empty((h, w), dtype=torch.float32))),
               (tq, ts, dict(status_out=torch.empty((h, w), dtype=torch.int32, device="cuda"))), (tq, ts, dict(depth=f32(h, w))), (tq, ts, dict(depth=f32(h, w + 1), bf=75.0)),
               (tq, ts, dict(depth=f32(h, w), bf=0.0)), (tq, ts, dict(stats=torch.empty((3,), dtype=torch.int32, device="cuda"))), (tq, ts, dict(min_region=0)), (tq, ts, dict(max_diff_q4=65536))]
        for x, y, kw in bad:
            with pytest.raises(vido.VidoError):
                ops.stereo_filter(x, y, **kw)
        _same(ctx.stereo_filter(q4, status, bf=75.0, **params), want)


def test_captured_graph_replayed_on_other_contents(vido, ctx):
    """The device form inside torch.cuda.graph (after one eager call of the size, which grows the scratch): replays on other contents equal the statement, counters included."""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    a = CASES.random_case(97, 130, 61); b = CASES.random_case(97, 130, 62)
    kw = dict(max_diff_q4=8, min_region=6)
    want_a, want_b = _want(*a, bf=75.0, **kw), _want(*b, bf=75.0, **kw)
    assert not np.array_equal(want_a[3], want_b[3])
    with limit(120, "capture and two replays"):
        tq, ts = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
        outs = [torch.zeros((97, 130), dtype=torch.float32, device="cuda"), torch.zeros((97, 130), dtype=torch.uint8, device="cuda"),
                torch.zeros((97, 130), dtype=torch.float32, device="cuda"), torch.zeros((4,), dtype=torch.int32, device="cuda")]
        run = lambda: ops.stereo_filter(tq, ts, out=outs[0], status_out=outs[1], depth=outs[2], stats=outs[3], bf=75.0, **kw)
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
            tq.copy_(torch.from_numpy(pair[0])); ts.copy_(torch.from_numpy(pair[1]))
            for o in outs:
                o.fill_(5)
            g.replay()
            torch.cuda.synchronize()
            _same(tuple(o.cpu().numpy() for o in outs), want)


def test_every_refusal_leaves_the_context_usable(vido, ctx):
    import torch
    name, q4, status, params, _ = ALL[6]                                                       # random 64 x 64
    assert q4.shape == (64, 64)
    with limit(120, "refusals"):
        good = ctx.stereo_filter(q4, status, bf=75.0, **params)
        lib = ctx.lib; f = lib.vido_stereo_filter
        disp = np.empty((64, 64), np.float32); st = np.empty((64, 64), np.uint8); depth = np.empty((64, 64), np.float32); stats = np.empty(4, np.int32)
        P = lambda x: x.ctypes.data_as(C.c_void_p)
        err = lambda: lib.vido_last_error(ctx.h).decode()
        call = lambda q=P(q4), s=P(status), w=64, h=64, t=8, m=6, bf=75.0, o=(P(disp), P(st), P(depth), P(stats)), dev=0: f(ctx.h, q, s, w, h, t, m, bf, *o, dev)
        assert call() == 0
        assert call(q=None) == -1 and "null image" in err()
        assert call(s=None) == -1 and "null image" in err()
        for w, h in ((0, 64), (64, 0), (4096, 64), (64, 4096), (-1, 64)):
            assert call(w=w, h=h) == -1 and "size" in err()
        for t in (-1, 65536):
            assert call(t=t) == -1 and "max_diff_q4" in err()
        for m in (0, -1, (1 << 24) + 1):
            assert call(m=m) == -1 and "min_region" in err()
        assert call(o=(None, None, None, None)) == -1 and "no output" in err()
        for bf in (0.0, -1.0, float("inf"), float("nan")):
            assert call(bf=bf) == -1 and "bf" in err()
            assert call(bf=bf, o=(P(disp), P(st), None, P(stats))) == 0                        # ignored without depth_out
        buf = np.zeros(64 * 64 + 64, np.uint8); buf[:64 * 64] = status.ravel()
        at = lambda off: C.c_void_p(buf.ctypes.data + off)
        for off in (1, 64, 64 * 63 - 1):                                                        # (63 rows: either image ends inside the buffer)
            assert call(s=at(0), h=63, o=(P(disp), at(off), P(depth), P(stats))) == -1 and "overlaps" in err()
            assert call(s=at(off), h=63, o=(P(disp), at(0), P(depth), P(stats))) == -1 and "overlaps" in err()
        assert call(s=at(0), o=(P(disp), at(0), P(depth), P(stats))) == 0 and np.array_equal(buf[:64 * 64].reshape(64, 64), good[1])
        tq, ts = torch.from_numpy(q4).cuda(), torch.from_numpy(status).cuda()
        t4 = [torch.zeros(64 * 64 + 1, dtype=torch.int32, device="cuda") for _ in range(4)]
        dp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
        for k in (0, 2, 3):                                                                     # device form, one misaligned 4-byte output: refused before any launch
            o = tuple(dp(t4[i], 2 if i == k else 0) for i in range(4))
            assert call(q=dp(tq), s=dp(ts), o=o, dev=1) == -1 and "aligned" in err()
        assert call(q=dp(tq, 2), s=dp(ts), w=63, o=tuple(dp(x) for x in t4), dev=1) == -1 and "aligned" in err()
        assert f(None, P(q4), P(status), 64, 64, 8, 6, 75.0, P(disp), P(st), P(depth), P(stats), 0) == -1
        with pytest.raises(vido.VidoError):
            ctx.stereo_filter(q4, status[:32])
        with pytest.raises(vido.VidoError):
            ctx.stereo_filter(q4.astype(np.int64), status)
        with pytest.raises(vido.VidoError):
            ctx.stereo_filter(q4, status, min_region=0)
        _same(ctx.stereo_filter(q4, status, bf=75.0, **params), good)
    _same(good, _want(q4, status, bf=75.0, **params))
