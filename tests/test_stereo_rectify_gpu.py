"""MI355X: vido_rectify (csrc/stereorectify.hip: k_rectify<1|3|4>) against the numpy statement (tests/refimpl/stereo_rectify_np.py): every image and every inside plane
bit for bit, no tolerance anywhere.  Shapes: destination widths 16, 17, 18, 19 (the four tails of the 4-pixel groups) x channels 1, 3, 4 x heights 16 and 17;
23 x 18 -> 37 x 16 and back; tight strides and strides padded by 1, 2, 3 bytes, images at a base offset of 1 byte inside larger tensors (every store path); one camera
and two cameras with different maps; hostile maps over sources that are slices of a buffer filled with 0xA5 (a read outside the source would show in an output that must
be 0); the host-staged and the device route; a captured graph replayed twice; every refusal; one 640 x 480 x 3 pair of the rig.  Around every device destination lie
guard bytes that must stay as they were.  The context is configured for 64 x 64: the op does not depend on that.  Each GPU step runs under limit()."""
import ctypes as C
import numpy as np
import pytest

from refimpl import stereo_rectify_np as G
from refimpl import stereo_rectify_cases as CASES
from test_detect_every_gpu import limit

pytestmark = pytest.mark.gpu

FILL_SRC, FILL_DST = 0xA5, 0x5A


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    yield c
    c.close()


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        assert False, (what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _embed(img, cn, pad, off, fill):
    """img [h, w(, cn)] -> (flat u8 buffer filled with `fill` that holds img's rows `w * cn + pad` bytes apart from byte `off` on, stride)"""
    h, w = img.shape[:2]
    stride = w * cn + pad
    buf = np.full(off + h * stride + 37, fill, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[off:], (h, w * cn), (stride, 1))
    rows[...] = img.reshape(h, w * cn)
    return buf, stride


def device_call(ctx, srcs, maps, src_pad=0, dst_pad=0, src_off=0, dst_off=0, inside=True):
    """vido_rectify's device form on the given sources / maps (one or two cameras): sources embedded in 0xA5 buffers, destinations in 0x5A buffers.
    -> [(out, inside)] per camera; asserts that every byte of a destination buffer outside the image's rows is untouched."""
    import torch
    cn = 1 if srcs[0].ndim == 2 else srcs[0].shape[2]
    sh, sw = srcs[0].shape[:2]; h, w = maps[0].shape[:2]
    dstride = w * cn + dst_pad
    tsrc, tmap, tdst, tins = [], [], [], []
    for s, m in zip(srcs, maps):
        buf, sstride = _embed(s, cn, src_pad, src_off, FILL_SRC)
        tsrc.append(torch.from_numpy(buf).cuda()); tmap.append(torch.from_numpy(np.ascontiguousarray(m)).cuda())
        tdst.append(torch.full((dst_off + h * dstride + 37,), FILL_DST, dtype=torch.uint8, device="cuda"))
        tins.append(torch.full((h * w + 8,), FILL_DST, dtype=torch.uint8, device="cuda") if inside else None)
    torch.cuda.synchronize()
    two = len(srcs) == 2
    ip = lambda k: None if tins[k] is None else tins[k].data_ptr()
    ctx.rectify_device(tsrc[0].data_ptr() + src_off, tmap[0].data_ptr(), tdst[0].data_ptr() + dst_off, cn, sstride, sw, sh, w, h, dstride,
                       src1_ptr=tsrc[1].data_ptr() + src_off if two else None, map1_ptr=tmap[1].data_ptr() if two else None, dst1_ptr=tdst[1].data_ptr() + dst_off if two else None,
                       inside0_ptr=ip(0), inside1_ptr=ip(1) if two else None)
    ctx.synchronize()
    res = []
    for k in range(len(srcs)):
        buf = tdst[k].cpu().numpy()
        rows = np.lib.stride_tricks.as_strided(buf[dst_off:], (h, w * cn), (dstride, 1))
        out = rows.copy().reshape((h, w) if srcs[0].ndim == 2 else (h, w, cn))
        guard = buf.copy(); np.lib.stride_tricks.as_strided(guard[dst_off:], (h, w * cn), (dstride, 1))[...] = FILL_DST
        assert (guard == FILL_DST).all(), ("a byte outside the destination's rows changed", k, np.argwhere(guard != FILL_DST)[:4].tolist())
        ins = None
        if inside:
            ib = tins[k].cpu().numpy()
            assert (ib[h * w:] == FILL_DST).all()
            ins = ib[:h * w].reshape(h, w)
        assert np.array_equal(tsrc[k].cpu().numpy(), _embed(srcs[k], cn, src_pad, src_off, FILL_SRC)[0])
        res.append((out, ins))
    return res


def _check(res, srcs, maps, what):
    for k, ((out, ins), s, m) in enumerate(zip(res, srcs, maps)):
        want, wins = G.rectify(s, m)
        _eq(out, want, (what, "camera", k))
        if ins is not None:
            _eq(ins, wins, (what, "inside", k))


@pytest.mark.parametrize("cn", (1, 3, 4))
def test_tails_heights_and_both_routes(ctx, cn):
    """16 .. 19 x 16 | 17 from a 23 x 18 source, two cameras with different maps: the device route and the host route give the statement's bytes"""
    with limit(120, "tails, %d channels" % cn):
        for w in (16, 17, 18, 19):
            for h in (16, 17):
                srcs = [CASES.image(23, 18, cn, 10 * w + h), CASES.image(23, 18, cn, 10 * w + h + 100)]
                maps = [CASES.smooth_map(23, 18, w, h, w + h), CASES.hostile_map(23, 18, w, h, w * h)[0]]
                _check(device_call(ctx, srcs, maps), srcs, maps, ("device", w, h, cn))
                o0, o1, i0, i1 = ctx.rectify(srcs[0], maps[0], srcs[1], maps[1])
                _check([(o0, i0), (o1, i1)], srcs, maps, ("host", w, h, cn))
                o0, i0 = ctx.rectify(srcs[1], maps[1])                                          # one camera
                _check([(o0, i0)], srcs[1:], maps[1:], ("host, one camera", w, h, cn))
                _check(device_call(ctx, srcs[:1], maps[:1], inside=False), srcs[:1], maps[:1], ("device, one camera, no inside plane", w, h, cn))


@pytest.mark.parametrize("cn", (1, 3, 4))
def test_strides_and_base_offsets(ctx, cn):
    """every store path: a destination row base that is 16-byte, 4-byte and not 4-byte aligned; sources at odd bases and strides"""
    with limit(120, "strides, %d channels" % cn):
        for (sw, sh, w, h) in ((23, 18, 37, 16), (37, 16, 23, 18), (16, 16, 20, 17)):
            srcs = [CASES.image(sw, sh, cn, sw + cn), CASES.image(sw, sh, cn, sw + cn + 50)]
            maps = [CASES.smooth_map(sw, sh, w, h, 7), CASES.planted_map(sw, sh, w, h)[0]]
            for dst_pad in (0, 1, 2, 3):
                for dst_off in (0, 1, 4, 16):
                    _check(device_call(ctx, srcs, maps, dst_pad=dst_pad, dst_off=dst_off), srcs, maps, ("dst", sw, sh, w, h, cn, dst_pad, dst_off))
            for src_pad, src_off in ((1, 0), (2, 1), (3, 3), (0, 1)):
                _check(device_call(ctx, srcs, maps, src_pad=src_pad, src_off=src_off), srcs, maps, ("src", sw, sh, w, h, cn, src_pad, src_off))
            # the host route with padded rows: the bytes between the rows come back as they were
            dbuf, dstride = _embed(np.zeros((h, w, cn), np.uint8), cn, 3, 0, FILL_DST)
            d0 = np.lib.stride_tricks.as_strided(dbuf, (h, w, cn) if cn > 1 else (h, w), (dstride, cn, 1) if cn > 1 else (dstride, 1))
            out, ins = ctx.rectify(srcs[0], maps[0], dst0=d0)
            _check([(np.ascontiguousarray(out), ins)], srcs[:1], maps[:1], ("host, padded dst", cn))
            guard = dbuf.copy(); np.lib.stride_tricks.as_strided(guard, (h, w * cn), (dstride, 1))[...] = FILL_DST
            assert (guard == FILL_DST).all()


def test_hostile_maps_read_nothing_outside_the_source(ctx):
    with limit(120, "hostile maps"):
        for cn in (1, 3, 4):
            for (sw, sh, w, h) in ((23, 18, 37, 16), (37, 16, 23, 18), (16, 16, 19, 17)):
                srcs = [CASES.image(sw, sh, cn, 3), CASES.image(sw, sh, cn, 4)]
                m0, census = CASES.hostile_map(sw, sh, w, h, 11 + cn)
                assert all(v > 0 for v in census.values()), census
                full = np.random.RandomState(5).randint(-2 ** 31, 2 ** 31, (h, w, 2), dtype=np.int64).astype(np.int32)     # uniform over the full int32 range
                planted, pairs = CASES.planted_map(sw, sh, w, h)
                for maps in ([m0, full], [planted, m0]):
                    for src_pad, src_off in ((0, 0), (5, 3)):
                        res = device_call(ctx, srcs, maps, src_pad=src_pad, src_off=src_off)
                        _check(res, srcs, maps, ("hostile", cn, sw, sh, w, h, src_pad))
                        for (out, ins) in res:
                            assert (out.reshape(h, w, -1)[ins == 0] == 0).all()
                # the planted pairs by name: the last inside value reads the corner pixel itself, the first outside value is 0
                out, ins = device_call(ctx, srcs[:1], [planted])[0]
                o = out.reshape(h, w, -1); s = srcs[0].reshape(sh, sw, -1)
                assert pairs[4] == ((sw - 1) * 256, (sh - 1) * 256) and ins[0, 4] == 1 and np.array_equal(o[0, 4], s[sh - 1, sw - 1])
                assert ins[0, 5] == 0 and ins[0, 6] == 0 and not o[0, 5].any() and not o[0, 6].any()
                assert ins[0, 0] == 0 and ins[0, 1] == 0 and ins[0, 2] == 0 and ins[0, 3] == 0 and ins[0, 7] == 1 and np.array_equal(o[0, 7], s[0, 0])


def test_hipops_form_and_captured_graph(vido, ctx):
    """HipOps.rectify on a side stream, then captured WITHOUT an eager call before it (the op has no scratch) and replayed twice with the sources changed in between"""
    import torch
    from vido_slam_amd import nets
    ops = nets.HipOps(ctx)
    sw, sh, w, h, cn = 37, 18, 23, 17, 3
    a = [CASES.image(sw, sh, cn, 21), CASES.image(sw, sh, cn, 22)]; b = [CASES.image(sw, sh, cn, 23), CASES.image(sw, sh, cn, 24)]
    maps = [CASES.smooth_map(sw, sh, w, h, 1), CASES.hostile_map(sw, sh, w, h, 2)[0]]
    with limit(120, "HipOps.rectify, capture and two replays"):
        tl, tr = torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda()
        ml, mr = torch.from_numpy(maps[0]).cuda(), torch.from_numpy(maps[1]).cuda()
        ol, orr = torch.zeros((h, w, cn), dtype=torch.uint8, device="cuda"), torch.zeros((h, w, cn), dtype=torch.uint8, device="cuda")
        il, ir = torch.zeros((h, w), dtype=torch.uint8, device="cuda"), torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                got = ops.rectify(tl, ml, tr, mr, out_left=ol, out_right=orr, inside_left=il, inside_right=ir)
        assert got[0] is ol and got[1] is orr
        torch.cuda.synchronize()
        for pair in (b, a):
            tl.copy_(torch.from_numpy(pair[0])); tr.copy_(torch.from_numpy(pair[1]))
            for o in (ol, orr, il, ir):
                o.fill_(9)
            g.replay()
            torch.cuda.synchronize()
            _check([(ol.cpu().numpy(), il.cpu().numpy()), (orr.cpu().numpy(), ir.cpu().numpy())], pair, maps, "replay")
        # eager forms: one camera returns a tensor, two a pair; new tensors when none are given; a grey image
        one = ops.rectify(tl, ml)
        two = ops.rectify(tl, ml, tr, mr)
        grey = torch.from_numpy(np.ascontiguousarray(a[0][..., 0])).cuda()
        og = ops.rectify(grey, mr)
        torch.cuda.synchronize()
        _eq(one.cpu().numpy(), G.rectify(a[0], maps[0])[0], "one"); _eq(two[1].cpu().numpy(), G.rectify(a[1], maps[1])[0], "two"); _eq(og.cpu().numpy(), G.rectify(a[0][..., 0], maps[1])[0], "grey")
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")
        bad = [dict(left=tl.cpu()), dict(map_left=ml.cpu()), dict(left=tl.float()), dict(map_left=ml.float()), dict(map_left=ml[..., 0]), dict(left=tl[:, ::2]), dict(right=tr),
               dict(right=tr, map_right=mr[:16].contiguous()), dict(right=tr[:, :30].contiguous(), map_right=mr), dict(map_right=mr), dict(out_right=u8(h, w, cn)),
               dict(inside_right=u8(h, w)), dict(out_left=u8(h, w)), dict(out_left=u8(h, w + 1, cn)), dict(inside_left=u8(h, w, 1)), dict(out_left=torch.empty((h, w, cn), dtype=torch.uint8)),
               dict(left=tl[None]), dict(left=u8(sh, sw, 2)), dict(out_left=tl[:h, :w].contiguous().int())]
        for kw in bad:
            with pytest.raises(vido.VidoError):
                ops.rectify(**{**dict(left=tl, map_left=ml), **kw})
        with pytest.raises(vido.VidoError):                                                       # an output that is an input
            ops.rectify(ol, torch.from_numpy(CASES.smooth_map(w, h, w, h, 1)).cuda(), out_left=ol)


def test_every_refusal_leaves_the_outputs_untouched(vido, ctx):
    import torch
    sw, sh, w, h, cn = 23, 18, 20, 16, 3
    srcs = [CASES.image(sw, sh, cn, 31), CASES.image(sw, sh, cn, 32)]
    maps = [CASES.smooth_map(sw, sh, w, h, 1), CASES.smooth_map(sw, sh, w, h, 2)]
    with limit(120, "refusals"):
        lib = ctx.lib; f = lib.vido_rectify
        outs = [np.full((h, w, cn), 77, np.uint8), np.full((h, w, cn), 77, np.uint8), np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)]
        P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        err = lambda: lib.vido_last_error(ctx.h).decode()
        def call(s0=P(srcs[0]), s1=P(srcs[1]), cn=cn, ss=sw * cn, sw=sw, sh=sh, m0=P(maps[0]), m1=P(maps[1]), w=w, h=h, d0=P(outs[0]), d1=P(outs[1]), ds=w * cn, i0=P(outs[2]), i1=P(outs[3]), dev=0):
            return f(ctx.h, s0, s1, cn, ss, sw, sh, m0, m1, w, h, d0, d1, ds, i0, i1, dev)
        untouched = lambda: all((o == 77).all() for o in outs)
        for kw in (dict(s0=None), dict(m0=None), dict(d0=None)):
            assert call(**kw) == -1 and "null" in err() and untouched(), kw
        for kw in (dict(s1=None), dict(m1=None), dict(d1=None), dict(s1=None, m1=None), dict(s1=None, d1=None), dict(m1=None, d1=None)):
            assert call(**kw) == -1 and "together" in err() and untouched(), kw
        assert call(s1=None, m1=None, d1=None) == -1 and "inside1_out" in err() and untouched()
        for c in (0, 2, 5, -1):
            assert call(cn=c) == -1 and "channels" in err() and untouched()
        assert call(ss=sw * cn - 1) == -1 and "stride" in err() and untouched()
        assert call(ds=w * cn - 1) == -1 and "stride" in err() and untouched()
        for kw in (dict(sw=15, ss=15 * cn), dict(sh=15), dict(w=15), dict(h=15), dict(sw=4096, ss=4096 * cn), dict(sh=4096), dict(w=4096, ds=4096 * cn), dict(h=4096), dict(w=-1)):
            assert call(**kw) == -1 and "size" in err() and untouched(), kw
        # a destination that overlaps a source: the first and the last byte of either, an inside plane over a map
        big = np.full(sh * sw * cn + h * w * cn, 77, np.uint8); big[:sh * sw * cn] = srcs[0].ravel()
        at = lambda off: C.c_void_p(big.ctypes.data + off)
        for off in (0, 1, sh * sw * cn - 1):
            assert call(s0=at(0), d0=at(off)) == -1 and "overlaps" in err()
            assert call(s1=at(0), d0=at(off)) == -1 and "overlaps" in err()
        assert call(s0=at(h * w * cn - 1), sh=16, d0=at(0)) == -1 and "overlaps" in err()
        assert call(i0=P(maps[1])) == -1 and "overlaps" in err()
        assert call(d1=P(outs[0])) == -1 and "are one" in err()
        assert np.array_equal(big[:sh * sw * cn], srcs[0].ravel()) and (big[sh * sw * cn:] == 77).all() and untouched()
        assert call(s0=at(0), d0=at(sh * sw * cn)) == 0 and np.array_equal(big[sh * sw * cn:].reshape(h, w, cn), G.rectify(srcs[0], maps[0])[0])      # adjacent is fine
        assert f(None, P(srcs[0]), None, cn, sw * cn, sw, sh, P(maps[0]), None, w, h, P(outs[0]), None, w * cn, None, None, 0) == -1
        # the device form: a map that is not 4-byte aligned is refused before any launch
        ts = torch.from_numpy(srcs[0]).cuda(); tm = torch.zeros(h * w * 2 + 1, dtype=torch.int32, device="cuda"); td = torch.full((h, w, cn), 77, dtype=torch.uint8, device="cuda")
        with pytest.raises(vido.VidoError, match="aligned"):
            ctx.rectify_device(ts.data_ptr(), tm.data_ptr() + 2, td.data_ptr(), cn, sw * cn, sw, sh, w, h, w * cn)
        torch.cuda.synchronize()
        assert bool((td == 77).all())
        for kw in (dict(src1=srcs[1]), dict(map1=maps[1]), dict(dst1=np.empty((h, w, cn), np.uint8))):
            with pytest.raises(vido.VidoError):
                ctx.rectify(srcs[0], maps[0], **kw)
        for a, m, kw in ((srcs[0].astype(np.int32), maps[0], {}), (srcs[0], maps[0].astype(np.int64), {}), (srcs[0], maps[0][..., 0], {}), (srcs[0], maps[0], dict(dst0=np.empty((h, w), np.uint8))),
                         (srcs[0], maps[0], dict(src1=srcs[1][:, :20], map1=maps[1])), (srcs[0], maps[0], dict(src1=srcs[1], map1=maps[1][:15]))):
            with pytest.raises(vido.VidoError):
                ctx.rectify(a, m, **kw)
        good = ctx.rectify(srcs[0], maps[0], srcs[1], maps[1])                                    # the context is still usable
        _check([(good[0], good[2]), (good[1], good[3])], srcs, maps, "after the refusals")


def test_rig_pair_640x480x3(vido, ctx):
    """One raw 640 x 480 x 3 pair of the rig (K_raw = (500, 500, 319.5, 239.5), P = (470, 470, 319.5, 239.5), the KAIST coefficients, about 1 degree per camera)"""
    import torch
    from vido_slam_amd import nets
    w, h = 640, 480
    P, K_raw = (470.0, 470.0, 319.5, 239.5), (500.0, 500.0, 319.5, 239.5)
    scene = vido.synth.Scene3D(n_frames=2, w=w, h=h, K=P, seed=3)
    raw_l, raw_r = scene.raw_stereo_frame(1, 0.5, K_raw, CASES.KAIST_DIST, CASES.R_LEFT, CASES.R_RIGHT)
    bgr = [vido.synth.gray_to_bgr(raw_l), vido.synth.gray_to_bgr(raw_r)]
    bgr[0][..., 1] = np.roll(bgr[0][..., 1], 1, 0); bgr[1][..., 2] = 255 - bgr[1][..., 2]                            # three different channels
    maps = [vido.rectify_map(K_raw, CASES.KAIST_DIST, R, P, (w, h), (w, h)) for R in (CASES.R_LEFT, CASES.R_RIGHT)]
    for (m, ins), R in zip(maps, (CASES.R_LEFT, CASES.R_RIGHT)):
        wm, wi = G.rectify_map(K_raw, CASES.KAIST_DIST, R, P, (w, h), (w, h))
        _eq(m, wm, "map"); _eq(ins, wi, "inside")
        assert 0.85 <= ins.mean() < 1.0
    with limit(120, "640 x 480 x 3 pair"):
        ops = nets.HipOps(ctx)
        tl, tr = torch.from_numpy(bgr[0]).cuda(), torch.from_numpy(bgr[1]).cuda()
        il, ir = torch.zeros((h, w), dtype=torch.uint8, device="cuda"), torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        ol, orr = ops.rectify(tl, torch.from_numpy(maps[0][0]).cuda(), tr, torch.from_numpy(maps[1][0]).cuda(), inside_left=il, inside_right=ir)
        torch.cuda.synchronize()
        _check([(ol.cpu().numpy(), il.cpu().numpy()), (orr.cpu().numpy(), ir.cpu().numpy())], bgr, [maps[0][0], maps[1][0]], "rig pair")
        _eq(il.cpu().numpy(), maps[0][1], "the map's own inside plane")
        host = ctx.rectify(bgr[0], maps[0][0], bgr[1], maps[1][0])
        _eq(host[0], ol.cpu().numpy(), "host route, left"); _eq(host[1], orr.cpu().numpy(), "host route, right")
