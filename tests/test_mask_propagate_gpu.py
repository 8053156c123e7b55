"""MI355X: vido_mask_propagate / vido_frame_propagate_mask (csrc/maskprop.hip) against the numpy statement of the rule (tests/refimpl/mask_propagate_np.py): bit-exact
label images and counters on hostile random inputs, degenerate images, a scene whose objects cross, the quality of a chained propagation on a rendered scene, refusals,
graph replay and the tracker's slot call.  Every reference image is computed once (REF) and never modified."""
import numpy as np
import pytest
import torch

from refimpl.mask_propagate_np import propagate, scatter_keys

pytestmark = pytest.mark.gpu

CTX_W, CTX_H = 1242, 375                       # the largest frame of the bit-exactness cases; the smaller ones run through the same context (and its one key plane)
SIZES = ((64, 64), (201, 151), (375, 1242))    # H, W
LABELS = (1, 254, 70000, 2, 37)
REF = {}


def blob_image(H, W, seed, labels=LABELS):
    """Random rectangles and discs of the given labels over zeros; a few pixels of labels <= 0 that must never scatter."""
    rng = np.random.RandomState(seed)
    m = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(12):
        lab = labels[i % len(labels)]
        cy, cx = rng.randint(0, H), rng.randint(0, W); ry, rx = rng.randint(3, max(4, H // 4)), rng.randint(3, max(4, W // 5))
        if i & 1:
            m[max(0, cy - ry):cy + ry, max(0, cx - rx):cx + rx] = lab
        else:
            m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = lab
    neg = rng.rand(H, W) < 0.01
    m[neg] = -rng.randint(1, 9, int(neg.sum()))
    return m


def hostile_inputs(H, W, seed):
    """mask, flow in +-12 px sprinkled with exact half-integers, NaN, +-inf, +-1e30 and +-32768, depth from a few values (equal-depth collisions happen) with zeros,
    negatives and NaN."""
    rng = np.random.RandomState(seed)
    m = blob_image(H, W, seed + 1)
    f = rng.uniform(-12, 12, (H, W, 2)).astype(np.float32)
    half = rng.rand(H, W, 2) < 0.15
    f[half] = (rng.randint(-12, 12, int(half.sum())) + 0.5).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, 32768.0, -32768.0):
        f[rng.rand(H, W, 2) < 0.004] = v
    d = rng.choice(np.array([1.0, 1.5, 2.0, 2.5, 7.25], np.float32), (H, W))
    for v in (0.0, -1.0, np.nan, -0.0, np.inf):
        d[rng.rand(H, W) < 0.01] = v
    return m, f, d.astype(np.float32)


def reference(key, make):
    if key not in REF:
        m, f, d = make()
        REF[key] = (m, f, d, propagate(m, f, d), propagate(m, f, None))
        for a in (m, f, d):
            a.setflags(write=False)
    return REF[key]


@pytest.fixture(scope="module")
def ops(vido):
    from vido_slam_amd import nets
    ctx = vido.Context(width=CTX_W, height=CTX_H, max_batch=1)
    yield nets.HipOps(ctx)
    torch.cuda.synchronize()
    ctx.close()


def run(ops, m, f, d):
    """-> (out, stats, mask read back) with out pre-filled with garbage"""
    tm, tf = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(f.copy()).cuda()      # (copies: the shared reference inputs are read-only)
    td = torch.from_numpy(d.copy()).cuda() if d is not None else None
    out = torch.full(m.shape, -559038737, dtype=torch.int32, device="cuda"); st = torch.full((3,), 12345, dtype=torch.int32, device="cuda")
    r = ops.mask_propagate(tm, tf, td, out=out, stats=st)
    assert r is out
    return out.cpu().numpy(), st.cpu().numpy(), tm.cpu().numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_bit_exact_on_hostile_inputs_with_and_without_depth(ops, H, W):
    """Two different inputs back to back through one context, each with and without depth: a key left behind by the call before would show in the next image."""
    for seed in (11, 12):
        m, f, d, with_d, without_d = reference((H, W, seed), lambda: hostile_inputs(H, W, seed + 100 * H))
        assert {1, 254, 70000} <= set(np.unique(m).tolist()) and (m < 0).any()
        for depth, (ro, rs) in ((d, with_d), (None, without_d)):
            out, st, m_after = run(ops, m, f, depth)
            print("%dx%d seed %d depth %s: stats %s, reference %s" % (H, W, seed, depth is not None, st.tolist(), rs.tolist()))
            assert np.array_equal(m_after, m)
            assert np.array_equal(out, ro), "%d pixels differ" % int((out != ro).sum())
            assert np.array_equal(st, rs)
        assert with_d[1][2] > 0 and with_d[1][0] > with_d[1][1] > 0       # holes were filled and sources collided in the case
        assert not np.array_equal(with_d[0], without_d[0])                # the depth decides some collisions


def test_degenerate_images(ops):
    H, W = 97, 131
    f = np.full((H, W, 2), 1.25, np.float32); f[..., 1] = -2.5
    out, st, _ = run(ops, np.zeros((H, W), np.int32), f, None)
    assert not out.any() and st.tolist() == [0, 0, 0]
    one = np.full((H, W), 9, np.int32)
    ro, rs = propagate(one, f, None)
    out, st, _ = run(ops, one, f, None)
    assert np.array_equal(out, ro) and np.array_equal(st, rs)
    assert (out == 9).sum() == (H - 2) * (W - 1) and st.tolist() == [(H - 2) * (W - 1), (H - 2) * (W - 1), 0]       # moved by (1, -2): one column and two rows are vacated


def crossing_scene(vido):
    """Two squares that cross in the image AND in depth: object 1 starts nearer (6 m) and recedes by 1 m per frame, object 2 starts farther (9 m) and approaches; object 1
    moves right, object 2 left.  In frame 1 object 1 is the nearer one, in frame 2 object 2 is."""
    return vido.synth.Scene3D(n_frames=4, w=320, h=240, K=(250.0, 250.0, 159.5, 119.5), seed=3, step=0.25, yaw_deg=0.4, obj_half=0.8,
                              objects=((-0.7, 0.3, 6.0, 0.25, 0.0, 1.0), (0.7, 0.2, 9.0, -0.25, 0.0, -1.0)))


def test_crossing_objects_bit_exact_and_both_win_collisions(ops, vido):
    """Frames 1 and 2 of the crossing scene, bit-exact against the reference.  On the pixels where sources of BOTH objects land, object 1 wins all of them in frame 1 (it is
    nearer there) and object 2 all of them in frame 2 (the depth order has swapped): each object beats the other label somewhere, by depth, not by label order."""
    scene = crossing_scene(vido)
    for k, winner in ((1, 1), (2, 2)):
        _, d, f, m = scene.frame(k)
        d = np.ascontiguousarray(d, np.float32); f = np.ascontiguousarray(f, np.float32)
        ro, rs = propagate(m, f, d)
        out, st, _ = run(ops, m, f, d)
        assert np.array_equal(out, ro) and np.array_equal(st, rs)
        H, W = m.shape                                                    # sources per target, per label
        ys, xs = np.nonzero(m > 0)
        tx = xs + np.rint(f[ys, xs, 0]).astype(np.int64); ty = ys + np.rint(f[ys, xs, 1]).astype(np.int64)
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        cnt = np.zeros((2, H * W), np.int64)
        for lab in (1, 2):
            s = ok & (m[ys, xs] == lab)
            np.add.at(cnt[lab - 1], ty[s] * W + tx[s], 1)
        cnt = cnt.reshape(2, H, W)
        both = (cnt[0] > 0) & (cnt[1] > 0)
        print("frame %d: %d targets with sources of both objects, %d taken by object 1, %d by object 2" % (k, int(both.sum()), int((out[both] == 1).sum()), int((out[both] == 2).sum())))
        assert both.sum() > 100 and (out[both] == winner).all()
        assert float(d[m == winner].mean()) < float(d[m == 3 - winner].mean())      # the winner is the nearer object of that frame


def test_chained_propagation_keeps_the_objects(ops, vido):
    """The 320 x 240 scene the rule was prototyped on: frame 0's true mask through flows 0 and 1 against frame 2's true mask, per-object IoU >= 0.90 (the numpy reference
    alone gives 0.941 or better here)."""
    scene = vido.synth.Scene3D(n_frames=4, w=320, h=240, K=(250.0, 250.0, 159.5, 119.5), seed=3, step=0.25, yaw_deg=0.4, obj_half=0.8,
                               objects=((-2.0, 0.3, 6.0, 0.12, 0, 0), (1.6, 0.2, 9.0, -0.10, 0, 0.25), (0.1, -1.2, 12.0, 0, 0, 0.30)))
    fr = [scene.frame(k) for k in range(3)]
    cur = torch.as_tensor(fr[0][3]).cuda(); ref = fr[0][3]
    for k in (0, 1):
        f = np.ascontiguousarray(fr[k][2], np.float32); d = np.ascontiguousarray(fr[k][1], np.float32)
        cur = ops.mask_propagate(cur, torch.as_tensor(f).cuda(), torch.as_tensor(d).cuda())
        ref = propagate(ref, f, d)[0]
        assert np.array_equal(cur.cpu().numpy(), ref)
    got, true = cur.cpu().numpy(), fr[2][3]
    for lab in (1, 2, 3):
        iou = ((got == lab) & (true == lab)).sum() / max(((got == lab) | (true == lab)).sum(), 1)
        print("object %d: IoU %.4f after two steps (%d true pixels)" % (lab, iou, int((true == lab).sum())))
        assert (true == lab).sum() > 100 and iou >= 0.90


def test_refusals(ops, vido):
    from vido_slam_amd.host import VidoError
    m = torch.zeros((64, 64), dtype=torch.int32, device="cuda"); f = torch.zeros((64, 64, 2), device="cuda")
    with pytest.raises(VidoError):
        ops.mask_propagate(m, f, out=m)
    with pytest.raises(VidoError):
        ops.mask_propagate(m.cpu(), f)
    with pytest.raises(VidoError):
        ops.mask_propagate(m, f.cpu())
    with pytest.raises(VidoError):
        ops.mask_propagate(m.to(torch.int64), f)
    with pytest.raises(VidoError):
        ops.mask_propagate(m, f.double())
    with pytest.raises(VidoError):
        ops.mask_propagate(m, f, depth=torch.zeros((64, 64), dtype=torch.float16, device="cuda"))
    with pytest.raises(VidoError):
        ops.mask_propagate(m, f[:, :, :1].expand(64, 64, 2))              # not contiguous
    with pytest.raises(VidoError):
        ops.mask_propagate(m, torch.zeros((64, 63, 2), device="cuda"))
    big = torch.zeros((CTX_H + 1, CTX_W), dtype=torch.int32, device="cuda")
    with pytest.raises(VidoError) as e:
        ops.mask_propagate(big, torch.zeros((CTX_H + 1, CTX_W, 2), device="cuda"))
    assert e.value.code == -1                                             # VIDO_E_INVALID, from the library
    # the C entry point itself: aliasing and null maps
    import ctypes as C
    ctx = ops.ctx
    o = torch.empty_like(m)
    assert ctx.lib.vido_mask_propagate(ctx.h, C.c_void_p(m.data_ptr()), C.c_void_p(f.data_ptr()), None, 64, 64, C.c_void_p(m.data_ptr()), None) == -1
    assert ctx.lib.vido_mask_propagate(ctx.h, None, C.c_void_p(f.data_ptr()), None, 64, 64, C.c_void_p(o.data_ptr()), None) == -1
    assert ctx.lib.vido_mask_propagate(ctx.h, C.c_void_p(m.data_ptr()), None, None, 64, 64, C.c_void_p(o.data_ptr()), None) == -1
    assert ctx.lib.vido_mask_propagate(ctx.h, C.c_void_p(m.data_ptr()), C.c_void_p(f.data_ptr()), None, 64, 64, None, None) == -1
    assert ctx.lib.vido_mask_propagate(ctx.h, C.c_void_p(m.data_ptr()), C.c_void_p(f.data_ptr()), None, 0, 64, C.c_void_p(o.data_ptr()), None) == -1
    # and a good call still works afterwards
    assert not ops.mask_propagate(m, f).any().item()


def test_graph_replay_equals_eager(ops):
    H, W = 201, 151
    cases = [reference((H, W, seed), lambda: hostile_inputs(H, W, seed + 100 * H)) for seed in (11, 12)]
    sm = torch.zeros((H, W), dtype=torch.int32, device="cuda"); sf = torch.zeros((H, W, 2), device="cuda"); sd = torch.ones((H, W), device="cuda")
    so = torch.zeros((H, W), dtype=torch.int32, device="cuda"); ss = torch.zeros((3,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.mask_propagate(sm, sf, sd, out=so, stats=ss)                  # the warm-up call: the key plane exists before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_propagate(sm, sf, sd, out=so, stats=ss)
    for m, f, d, (ro, rs), _ in cases:
        sm.copy_(torch.from_numpy(m.copy())); sf.copy_(torch.from_numpy(f.copy())); sd.copy_(torch.from_numpy(d.copy()))
        so.fill_(-7); ss.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager_out, eager_st, _ = run(ops, m, f, d)
        assert np.array_equal(so.cpu().numpy(), eager_out) and np.array_equal(ss.cpu().numpy(), eager_st)
        assert np.array_equal(eager_out, ro) and np.array_equal(eager_st, rs)


def test_slot_call_equals_reference_on_read_back_maps(vido):
    """Two frames of a scene uploaded into the tracker's slots (KITTI depth pre-scale: the slot holds bf / d), then the slot call: slot 1's mask == the reference on slot 0's
    read-back mask, flow and pre-scaled depth."""
    from vido_slam_amd import host
    scene = crossing_scene(vido)
    H, W = scene.h, scene.w
    ctx = vido.Context(width=W, height=H, max_batch=2)
    ff = host.FrameFeatures(ctx, host.track_params(dataset=1, fx=250.0, fy=250.0, cx=159.5, cy=119.5))
    for slot, k in ((0, 1), (1, 2)):
        _, d, f, m = scene.frame(k)
        ff.upload(slot, np.ascontiguousarray(d, np.float32).copy(), np.ascontiguousarray(f, np.float32), np.ascontiguousarray(m, np.int32))
    d0, f0, m0 = ff.read_maps(0)
    before1 = ff.read_maps(1)[2].copy()
    ro, rs = propagate(np.ascontiguousarray(m0.reshape(H, W)), np.ascontiguousarray(f0.reshape(H, W, 2)), np.ascontiguousarray(d0.reshape(H, W)))
    st = ctx.frame_propagate_mask(0, 1)
    d1, f1, m1 = ff.read_maps(1)
    assert np.array_equal(m1.reshape(H, W), ro) and list(st) == rs.tolist()
    assert not np.array_equal(m1, before1)                                # the slot's mask was replaced
    assert np.array_equal(ff.read_maps(0)[2], m0)                         # the source slot is untouched
    from vido_slam_amd.host import VidoError
    for a, b in ((0, 0), (-1, 1), (0, 2), (5, 0)):
        with pytest.raises(VidoError):
            ctx.frame_propagate_mask(a, b)
    ctx.close()
