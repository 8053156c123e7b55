"""GPU parity of the front-end list kernels (csrc/track.hip) where tests/test_track_gpu.py does not look: dataset frame sizes (pixel counts that are not a
multiple of 4, odd slot offsets, ragged lattices), hostile maps (tests/refimpl/hostile.py), list lengths around the 1024-thread rounds of the ordered
compaction, dense steps other than 4, UpdateMask's sequential rule, the point-samples entry, the copy route of the per-point calls.
Everything is compared with np.array_equal against oracle/track_oracle.c (NaN depth compares equal to NaN depth; nothing has a tolerance); the oracle itself is
pinned to the numpy reference by tests/test_track_ref_cpu.py.

Each test fails on a kernel that is subtly wrong.  One-line mutations of track.hip that were built as variant libraries and run against this module:
  * block_ordered_slot without `base += total`                  -> test_keypoint_counts (all seven), test_upload_and_lists, test_dense_step, test_every_probe_survives_and_none,
                                                                   test_update_mask_sequential_rule (its sample list is wrong already): 45 tests fail
  * k_dense_sample `j + fx >= 0` for `> 0`                      -> test_upload_and_lists at every size, test_keypoint_counts, test_dense_step (flow landing exactly on x = 0): 41 fail
  * vido_update_mask with `scattered = false` (no re-sample)    -> test_update_mask_sequential_rule at both sizes and test_per_point_calls_and_copy_route, nothing else
The small odd size is 201 x 151 (30 351 pixels, odd): vido_create accepts sizes from 64 x 64, but UpdateMask's five-object scene needs 201 x 151."""
import ctypes as C
import numpy as np
import pytest
import torch   # before the first Context: torch bundles its own HIP runtime and must be the one the process initialises
from refimpl import hostile, track_np

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)
TH_BG, TH_OBJ = hostile.TH_BG, hostile.TH_OBJ
N_LEVELS = {(640, 192): 5, (201, 151): 4}          # short frames: the top pyramid levels would be smaller than one FAST cell row (as in test_pipeline_gpu.py)
SIZES = pytest.mark.parametrize("size", hostile.SIZES, ids=lambda s: "%dx%d" % s)
KITTI, SMALL = (1242, 375), (201, 151)
CAM = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def all_eq(xs, ys):
    return len(xs) == len(ys) and all(eq(x, y) for x, y in zip(xs, ys))


@pytest.fixture(scope="module")
def ctx_of(vido):
    cache = {}
    def get(size):
        if size not in cache:
            cache[size] = vido.Context(width=size[0], height=size[1], max_batch=3, n_levels=N_LEVELS.get(size, 8))
        return cache[size]
    yield get
    for c in cache.values():
        c.close()


def params(vido, dataset=0, dense_step=4):
    return vido.track_params(dataset=dataset, depth_map_factor=5.0 if dataset else 1.0, bf=387.57, kaist_scale=1.2 if dataset == 2 else 1.0,
                             th_depth_bg=TH_BG, th_depth_obj=TH_OBJ, dense_step=dense_step, **CAM)


def batch(size, n_frames, dataset, n_kp, first=0):
    """hostile frames SEEDS[first:first+n_frames] as one batch -> raw depth, flow, mask, keypoints (n, n_kp).  Datasets 1 and 2 get a disparity-like raw
    depth (positive finite entries only: 0, negatives and NaN stay) so that bf / (d / f) lands in metric range."""
    fr = [hostile.frame(s, size[0], size[1], n_kp) for s in SEEDS[first:first + n_frames]]
    raw = np.stack([f[0] for f in fr]).copy()
    if dataset:
        pos = raw > 0
        raw[pos] = (387.57 * 5.0 / np.maximum(raw[pos], 0.5)).astype(np.float32)
    return raw, np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr]), np.stack([f[3] for f in fr])


def prescaled(oracle, raw, p):
    return np.stack([oracle.depth_prescale(d, p.dataset, p.depth_map_factor, p.bf, p.kaist_scale) for d in raw])


def check_lists(oracle, out, f, kps, depth, flow, mask, step=4, min_stat=0, min_obj=0):
    ref = oracle.static_candidates(kps, depth, flow, mask, TH_BG)
    n = out["n_stat"][f]
    assert n == len(ref[0]) and n >= min_stat, (n, len(ref[0]))
    assert all_eq([out[k][f, :n] for k in ("stat_idx", "stat_corr", "stat_flow", "stat_depth")], ref)
    ref = oracle.dense_object_samples(depth, flow, mask, TH_OBJ, step=step)
    n = out["n_obj"][f]
    assert n == len(ref[0]) and n >= min_obj, (n, len(ref[0]))
    assert all_eq([out[k][f, :n] for k in ("obj_keys", "obj_corr", "obj_depth", "obj_label", "obj_flow")], ref)


@SIZES
@pytest.mark.parametrize("n_frames,slot0,dataset", [(3, 0, 0), (2, 1, 1), (1, 2, 2), (1, 1, 0), (2, 0, 2), (1, 0, 1)])
def test_upload_and_lists(vido, oracle, ctx_of, size, n_frames, slot0, dataset):
    """upload + features of 1, 2 and 3 hostile frames at slot0 0, 1 and 2, all three depth conventions.  At 1242 x 375, 1241 x 376 and 201 x 151 the pixel count is
    not a multiple of 4: such a batch used to be refused, and slot 1 / slot 2 of the context's own maps start 8 bytes off a 16-byte boundary there."""
    ctx = ctx_of(size); p = params(vido, dataset); ff = vido.FrameFeatures(ctx, p)
    raw, flow, mask, kps = batch(size, n_frames, dataset, ctx.max_kp)
    if dataset == 0:
        for s in SEEDS[:n_frames]:
            hostile.check_hostile(s, size[0], size[1], ctx.max_kp)         # every hostile case >= 20 times, >= 50 static and >= 100 object survivors
    ref_depth = prescaled(oracle, raw, p)
    depth = raw.copy()
    ff.upload(slot0, depth, flow, mask)
    assert eq(depth, ref_depth)                                             # the caller's buffer is rescaled in place
    for f in range(n_frames):
        assert all_eq(ff.read_maps(slot0 + f), (ref_depth[f], flow[f], mask[f]))
    n_kps = np.full(n_frames, ctx.max_kp, np.int32)
    out = ff.features(slot0, kps, n_kps)
    for f in range(n_frames):
        check_lists(oracle, out, f, kps[f], ref_depth[f], flow[f], mask[f], min_stat=50, min_obj=100)
    if dataset == 0:                                                        # and once directly against the numpy reference
        n = out["n_obj"][0]
        assert all_eq([out[k][0, :n] for k in ("obj_keys", "obj_corr", "obj_depth", "obj_label", "obj_flow")],
                      track_np.dense_object_samples(track_np.depth_prescale(raw[0], 0, 1.0, 1.0, 1.0), flow[0], mask[0], TH_OBJ))


def test_features_refuses_a_non_contiguous_batch(vido, ctx_of):
    """slots 0 and 1 of a context filled by two aliased single frames that do not follow each other in memory: a 2-frame features call must refuse them,
    and the context stays usable."""
    ctx = ctx_of(SMALL); p = params(vido); ff = vido.FrameFeatures(ctx, p)
    raw, flow, mask, kps = batch(SMALL, 2, 0, ctx.max_kp)
    dev = [[torch.from_numpy(a[f].copy()).cuda() for a in (raw, flow, mask)] for f in (1, 0)]      # frame 1 allocated first: slot 1 cannot sit px floats behind slot 0
    for slot, (d, fl, m) in zip((1, 0), dev):
        ctx._check(ctx.lib.vido_frame_upload(ctx.h, slot, 1, C.c_void_p(d.data_ptr()), C.c_void_p(fl.data_ptr()), C.c_void_p(m.data_ptr()), 2, C.byref(p)))
    ctx.synchronize()
    assert dev[1][0].data_ptr() + raw[0].nbytes != dev[0][0].data_ptr()
    with pytest.raises(vido.VidoError) as e:
        ff.features(0, kps, np.full(2, 100, np.int32))
    assert e.value.code == -1
    depth = raw.copy(); ff.upload(0, depth, flow, mask)
    assert ff.features(0, kps, np.full(2, 100, np.int32))["n_obj"].min() >= 100


@pytest.mark.parametrize("size", [KITTI, (1280, 560)], ids=lambda s: "%dx%d" % s)
def test_frontend_batch_routes(vido, oracle, ctx_of, size):
    """vido_frontend_batch with host maps, device maps copied in, and device maps aliased, on three hostile frames; then ONE 1242 x 375-class frame at slot 1
    through the host route and through the alias route with map pointers that are only 4-byte aligned."""
    from vido_slam_amd import synth
    w, h = size; ctx = ctx_of(size); p = params(vido); ff = vido.FrameFeatures(ctx, p)
    gray = np.ascontiguousarray(np.stack([synth.make_frame(w, h, seed=s) for s in (1, 2, 3)]))      # the device routes hand over a raw pointer with strides (h w, w)
    raw, flow, mask, _ = batch(size, 3, 0, ctx.max_kp)
    ref_depth = prescaled(oracle, raw, p)
    kps, desc, cnt = ctx.orb_extract_batch(gray, want_desc=True)
    assert cnt.min() > 500

    def check(out, depth_after, frames):
        assert eq(depth_after, ref_depth[frames])
        assert np.array_equal(out["n_kp"], cnt[frames])
        for i, f in enumerate(frames):
            n = cnt[f]
            assert np.array_equal(out["kps"][i, :n], kps[f, :n]) and np.array_equal(out["desc"][i, :n], desc[f, :n])
            check_lists(oracle, out, i, kps[f, :n], ref_depth[f], flow[f], mask[f], min_stat=50, min_obj=100)

    all3 = [0, 1, 2]
    d = raw.copy(); check(ff.frontend_batch(0, gray, d, flow, mask), d, all3)
    g = torch.from_numpy(gray).cuda(); fl = torch.from_numpy(flow).cuda(); mk = torch.from_numpy(mask).cuda()
    gdesc = (g.data_ptr(), 3, h, w, h * w, w)
    dd = torch.from_numpy(raw.copy()).cuda()
    out = ff.frontend_batch(0, gdesc, dd.data_ptr(), fl.data_ptr(), mk.data_ptr()); torch.cuda.synchronize()
    check(out, dd.cpu().numpy(), all3)
    assert all_eq(ff.read_maps(2), (ref_depth[2], flow[2], mask[2]))
    dd2 = torch.from_numpy(raw.copy()).cuda()
    out = ff.frontend_batch(0, gdesc, dd2.data_ptr(), fl.data_ptr(), mk.data_ptr(), alias=True); torch.cuda.synchronize()
    check(out, dd2.cpu().numpy(), all3)
    assert all_eq(ff.read_maps(1), (ref_depth[1], flow[1], mask[1]))
    # one frame, slot 1
    d = raw[1:2].copy(); check(ff.frontend_batch(1, gray[1:2], d, flow[1:2], mask[1:2]), d, [1])
    assert all_eq(ff.read_maps(1), (ref_depth[1], flow[1], mask[1]))
    def off4(a, dtype):                                   # the same data 4 bytes into a fresh allocation
        t = torch.empty(a.size + 1, dtype=dtype, device="cuda"); t[1:] = torch.from_numpy(a.ravel().copy()).cuda()
        return t
    td, tf, tm = off4(raw[2], torch.float32), off4(flow[2], torch.float32), off4(mask[2], torch.int32)
    g2 = torch.from_numpy(gray[2:3].copy()).cuda()
    out = ff.frontend_batch(1, (g2.data_ptr(), 1, h, w, h * w, w), td.data_ptr() + 4, tf.data_ptr() + 4, tm.data_ptr() + 4, alias=True); torch.cuda.synchronize()
    check(out, td[1:].cpu().numpy().reshape(1, h, w), [2])
    assert all_eq(ff.read_maps(1), (ref_depth[2], flow[2], mask[2]))


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2048, "max_kp"])
def test_keypoint_counts(vido, oracle, ctx_of, n):
    """list lengths around the 1024-thread rounds of block_ordered_slot (its running `base`), the empty list and the full capacity: one frame (the plain-copy
    upload path) and as the middle frame of a batch of three (the strided path)."""
    ctx = ctx_of(KITTI); p = params(vido); ff = vido.FrameFeatures(ctx, p)
    n = ctx.max_kp if n == "max_kp" else n
    raw, flow, mask, kps = batch(KITTI, 3, 0, ctx.max_kp)
    depth = raw.copy(); ff.upload(0, depth, flow, mask)
    one = ff.features(1, kps[1:2], np.array([n], np.int32))
    check_lists(oracle, one, 0, kps[1, :n], depth[1], flow[1], mask[1], min_stat=50 if n >= 1023 else 0, min_obj=100)
    counts = np.array([1025, n, 1], np.int32)
    out = ff.features(0, kps, counts)
    for f in range(3):
        check_lists(oracle, out, f, kps[f, :counts[f]], depth[f], flow[f], mask[f], min_obj=100)
    with pytest.raises(vido.VidoError):
        ff.features(0, kps, np.array([1, ctx.max_kp + 1, 1], np.int32))


def test_every_probe_survives_and_none(vido, oracle, ctx_of):
    """frame 0: label everywhere, usable depth, small inward flow -> n_obj equals the whole lattice (311 x 94 at 1241 x 376: ragged in x) and no static candidate;
    frame 1: no label -> no object sample, every keypoint survives; frame 2: no usable depth -> both lists empty."""
    size = (1241, 376); w, h = size
    ctx = ctx_of(size); p = params(vido); ff = vido.FrameFeatures(ctx, p)
    kps = np.stack([hostile.keypoints(s, w, h, ctx.max_kp) for s in SEEDS])
    depth = np.full((3, h, w), 10, np.float32); depth[2] = 0
    flow = np.full((3, h, w, 2), 0.5, np.float32); flow[1] = -0.25
    mask = np.zeros((3, h, w), np.int32); mask[0] = 3; mask[2, ::2] = 1
    ff.upload(0, depth, flow, mask)
    out = ff.features(0, kps, np.full(3, ctx.max_kp, np.int32))
    lattice = ((w + 3) // 4) * ((h + 3) // 4)
    assert list(out["n_obj"]) == [lattice, 0, 0] and list(out["n_stat"]) == [0, ctx.max_kp, 0]
    for f in range(3):
        check_lists(oracle, out, f, kps[f], depth[f], flow[f], mask[f])


@pytest.mark.parametrize("size", [KITTI, SMALL], ids=lambda s: "%dx%d" % s)
def test_dense_step(vido, oracle, ctx_of, size):
    """steps 5 and 8 are accepted and follow the reference's loop; steps 1-3 need more probes than the lists hold: VIDO_E_INVALID, and the context goes on working."""
    ctx = ctx_of(size); ff = vido.FrameFeatures(ctx, params(vido))
    raw, flow, mask, kps = batch(size, 2, 0, ctx.max_kp)
    depth = raw.copy(); ff.upload(1, depth, flow, mask)
    n_kps = np.full(2, 1500, np.int32)
    for step in (5, 1, 8, 2, 3, 4):
        ff.p = params(vido, dense_step=step)
        if step < 4:
            with pytest.raises(vido.VidoError) as e:
                ff.features(1, kps, n_kps)
            assert e.value.code == -1
            continue
        out = ff.features(1, kps, n_kps)
        for f in range(2):
            check_lists(oracle, out, f, kps[f, :1500], depth[f], flow[f], mask[f], step=step, min_stat=50, min_obj=20)


def upload_pair(ff, depth, flow_last, mask_last, mask_cur):
    """slot 0: the last frame, slot 1: the current one (its flow plays no part in UpdateMask)"""
    d = np.stack([depth, depth]).copy()
    ff.upload(0, d, np.stack([flow_last, np.zeros_like(flow_last)]), np.stack([mask_last, mask_cur]))


@pytest.mark.parametrize("size", [KITTI, SMALL], ids=lambda s: "%dx%d" % s)
def test_update_mask_sequential_rule(vido, oracle, ctx_of, size):
    """three lost labels (and a fourth that depends on the third): label 2's vote flips from 0 to 1 once label 1 has been scattered, label 3 is recovered in the
    round after the re-sample, label 5 flips on label 3's scatter.  Then cap = 1 with two labels recovered: the count says 2, one entry is written."""
    w, h = size; ctx = ctx_of(size); ff = vido.FrameFeatures(ctx, params(vido))
    s = hostile.um_sequential_scene(w, h)
    upload_pair(ff, s["depth"], s["flow_last"], s["mask_last"], s["mask_cur"])
    out = ff.features(0, np.zeros((1, 8), hostile.KP_DTYPE), np.zeros(1, np.int32))
    n = out["n_obj"][0]; lab, corr = out["obj_label"][0, :n].copy(), out["obj_corr"][0, :n].copy()
    assert n == 5 * 144
    ref_mask, ref_rec = oracle.update_mask(lab, corr, s["mask_last"], s["flow_last"], s["mask_cur"])
    np_mask, np_rec = track_np.update_mask(lab, corr, s["mask_last"], s["flow_last"], s["mask_cur"])
    rec = ff.update_mask(0, 1, lab, corr)
    assert list(rec) == list(ref_rec) == list(np_rec) == [1, 3]
    got = ff.read_maps(1)[2]
    assert np.array_equal(got, ref_mask) and np.array_equal(got, np_mask)
    upload_pair(ff, s["depth"], s["flow_last"], s["mask_last"], s["mask_cur"])
    lab = np.ascontiguousarray(lab, np.int32); corr = np.ascontiguousarray(corr, np.float32)
    two = np.full(4, -77, np.int32); nrec = C.c_int32(-1)
    ctx._check(ctx.lib.vido_update_mask(ctx.h, 0, 1, lab.ctypes.data_as(C.c_void_p), corr.ctypes.data_as(C.c_void_p), len(lab), two.ctypes.data_as(C.c_void_p), 1, C.byref(nrec)))
    assert nrec.value == 2 and list(two) == [1, -77, -77, -77]
    assert np.array_equal(ff.read_maps(1)[2], ref_mask)


@pytest.mark.parametrize("size", [KITTI, SMALL], ids=lambda s: "%dx%d" % s)
def test_update_mask_edges(vido, oracle, ctx_of, size):
    """exactly 100 in-image samples (taken) against 99 (skipped), an exact tie between 0 and a label (0 wins), scatter targets on the last row / column (written),
    past them and on row / column 0 (refused)."""
    w, h = size; ctx = ctx_of(size); ff = vido.FrameFeatures(ctx, params(vido))
    s = hostile.um_edge_scene(w, h)
    upload_pair(ff, np.full((h, w), 10, np.float32), s["flow_last"], s["mask_last"], s["mask_cur"])
    ref_mask, ref_rec = oracle.update_mask(s["last_label"], s["last_corr"], s["mask_last"], s["flow_last"], s["mask_cur"])
    np_mask, np_rec = track_np.update_mask(s["last_label"], s["last_corr"], s["mask_last"], s["flow_last"], s["mask_cur"])
    rec = ff.update_mask(0, 1, s["last_label"], s["last_corr"])
    assert list(rec) == list(ref_rec) == list(np_rec) == [7, 9, 10, 11]
    got = ff.read_maps(1)[2]
    assert np.array_equal(got, ref_mask) and np.array_equal(got, np_mask)
    assert (got[h - 1, w - 18:] == 10).all() and (got[0] == 0).all() and (got[1, 1:18] == 11).all()


def sample_points(w, h):
    """inside, on every border, negative fractions in (-1, 0), at w and h, far outside"""
    rng = np.random.RandomState(3)
    p = np.stack([rng.uniform(0, w, 1000), rng.uniform(0, h, 1000)], 1)
    xs = [0, 0.5, 1, 1.25, -0.25, -0.999, -1, -1.5, w - 2, w - 1.5, w - 1, w - 0.5, w, w + 0.5, -1e6, 1e6]
    ys = [0, 0.5, 1, 1.25, -0.25, -0.999, -1, -1.5, h - 2, h - 1.5, h - 1, h - 0.5, h, h + 0.5, -1e6, 1e6]
    return np.concatenate([p, np.array([(x, y) for x in xs for y in ys])]).astype(np.float32)


@pytest.mark.parametrize("size", [KITTI, SMALL], ids=lambda s: "%dx%d" % s)
def test_point_samples(vido, ctx_of, size):
    """vido_gather_point_samples against the rule of tests/test_track_ref_cpu.py::test_point_samples_rule, on slot 2 of hostile maps; n = 0; n past the capacity
    include/vido_c.h documents."""
    w, h = size; ctx = ctx_of(size); ff = vido.FrameFeatures(ctx, params(vido))
    raw, flow, mask, _ = batch(size, 1, 0, ctx.max_kp, first=2)
    depth = raw.copy(); ff.upload(2, depth, flow, mask)
    pts = sample_points(w, h)
    ref = track_np.point_samples(pts, depth[0], flow[0], mask[0])
    assert all_eq(ff.gather_point_samples(2, pts), ref)
    assert (ref[0] != 0).sum() > 100 and np.isnan(ref[1]).any()
    for k in (1, 255, 256, 257):
        assert all_eq(ff.gather_point_samples(2, pts[-k:]), [r[-k:] for r in ref])
    m, d, f = ff.gather_point_samples(2, np.zeros((0, 2), np.float32))
    assert len(m) == len(d) == len(f) == 0
    cap = 2 * max(ctx.max_kp, ((w + 3) // 4) * ((h + 3) // 4))
    big = np.resize(pts, (cap + 3, 2))
    assert all_eq(ff.gather_point_samples(2, big[:cap]), track_np.point_samples(big[:cap], depth[0], flow[0], mask[0]))
    with pytest.raises(vido.VidoError) as e:
        ff.gather_point_samples(2, big)
    assert e.value.code == -1
    assert all_eq(ff.gather_point_samples(2, pts), ref)


def per_point_calls(vido, oracle, ctx, size):
    """every per-point entry on one context -> list of result arrays (each already compared with the oracle / the numpy reference)"""
    w, h = size; p = params(vido); ff = vido.FrameFeatures(ctx, p)
    raw, flow, mask, kps = batch(size, 2, 0, ctx.max_kp)
    depth = raw.copy(); ff.upload(0, depth, flow, mask)
    res = []
    corr = oracle.dense_object_samples(depth[0], flow[0], mask[0], TH_OBJ)[1]
    keys = np.concatenate([corr, oracle.static_candidates(kps[0], depth[0], flow[0], mask[0], TH_BG)[1], sample_points(w, h)])
    res.append(ff.gather_static_depth(1, keys)); assert eq(res[-1], oracle.gather_static_depth(keys, depth[1]))
    res += ff.gather_object_depth_label(1, keys); assert all_eq(res[-2:], oracle.gather_object_depth_label(keys, depth[1], mask[1], TH_OBJ))
    res += ff.gather_point_samples(1, keys); assert all_eq(res[-3:], track_np.point_samples(keys, depth[1], flow[1], mask[1]))
    for n in (1, 257, 1000, 4099):                            # n = 1 and n not a multiple of the 256-thread workgroups
        s = hostile.points_scene(n, n, w, h)
        xw = ff.unproject_world(s["keys"], s["z"], s["Tcw"])
        assert eq(xw, oracle.unproject_world(s["keys"], s["z"], p.fx, p.fy, p.cx, p.cy, s["Tcw"])) and eq(xw, track_np.unproject_world(s["keys"], s["z"], p.fx, p.fy, p.cx, p.cy, s["Tcw"]))
        assert not np.isnan(xw).any() and (n == 1 or np.abs(xw).max() > 5e3)
        xc = ff.unproject_world(s["keys"] + np.float32(1.5), np.abs(s["z"]), np.eye(4, dtype=np.float32))
        f3, ol = ff.scene_flow(xw, xc, s["sem_last"], s["sem_cur"], s["obj_label"])
        assert all_eq((f3, ol), oracle.scene_flow(xw, xc, s["sem_last"], s["sem_cur"], s["obj_label"]))
        assert (ol[(s["sem_last"] <= 0) | (s["sem_cur"] <= 0)] == -1).all()
        res += [xw, xc, f3, ol]
    sc = hostile.um_sequential_scene(w, h)
    upload_pair(ff, sc["depth"], sc["flow_last"], sc["mask_last"], sc["mask_cur"])
    _, corr, _, lab, _ = oracle.dense_object_samples(sc["depth"], sc["flow_last"], sc["mask_last"], TH_OBJ)
    res.append(ff.update_mask(0, 1, lab, corr)); res.append(ff.read_maps(1)[2])
    ref_mask, ref_rec = oracle.update_mask(lab, corr, sc["mask_last"], sc["flow_last"], sc["mask_cur"])
    assert list(res[-2]) == list(ref_rec) == [1, 3] and np.array_equal(res[-1], ref_mask)
    return res


def test_per_point_calls_and_copy_route(vido, oracle, ctx_of, monkeypatch):
    """both gathers, point samples, back-projection (z of 0, negative, NaN; a pose 1e4 away), scene flow (labels 0 and below) and UpdateMask on the default
    zero-copy context, then on a fresh context created under VIDO_TRACK_IO_COPIES=1 (read once per context): the same bits."""
    zero_copy = per_point_calls(vido, oracle, ctx_of(KITTI), KITTI)
    monkeypatch.setenv("VIDO_TRACK_IO_COPIES", "1")
    ctx = vido.Context(width=KITTI[0], height=KITTI[1], max_batch=3)
    try:
        copies = per_point_calls(vido, oracle, ctx, KITTI)
    finally:
        ctx.close()
    assert all_eq(zero_copy, copies)
