"""CPU: the two witnesses of the tracking front end agree.  tests/refimpl/track_np.py (numpy, written from the reference lines) and
oracle/track_oracle.c (C) must give the same bits on the hostile inputs of tests/refimpl/hostile.py at every frame size the GPU parity
tests (tests/test_track_edges_gpu.py) use — every GPU assertion rests on the oracle, and this is what the oracle rests on.
Also here: the census of the committed seeds (a seed that drifts cannot make the GPU tests vacuous) and the point-samples rule as a specification."""
import numpy as np
import pytest
from refimpl import hostile, track_np

N_KP = 4256                      # 2 * n_features + 256 of the default context
SEEDS = (11, 12, 13)             # one per frame of a 3-frame batch
TH_BG, TH_OBJ = hostile.TH_BG, hostile.TH_OBJ
SIZES = pytest.mark.parametrize("size", hostile.SIZES, ids=lambda s: "%dx%d" % s)


def bits(a, b):
    """bit-for-bit: same dtype, same shape, same bytes (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def all_bits(xs, ys):
    return len(xs) == len(ys) and all(bits(x, y) for x, y in zip(xs, ys))


@SIZES
def test_committed_seeds_are_hostile(size):
    """every case of the generator's docstring occurs >= 20 times where it matters, and >= 50 static / >= 100 object entries survive"""
    for seed in SEEDS:
        c = hostile.check_hostile(seed, size[0], size[1], N_KP)
        assert len(c) == 33 and min(c.values()) >= 20, c


@SIZES
@pytest.mark.parametrize("dataset", [0, 1, 2])
def test_depth_prescale(oracle, size, dataset):
    raw = hostile.frame(SEEDS[dataset], size[0], size[1], N_KP)[0]
    factor, bf, scale = (1.0, 387.57, 1.0) if dataset == 0 else (5.0, 387.57, 1.2)
    ref = oracle.depth_prescale(raw, dataset, factor, bf, scale)
    assert bits(track_np.depth_prescale(raw, dataset, factor, bf, scale), ref)
    assert np.isnan(ref).sum() >= 20 and (ref[raw < 0] == 0).all() and (raw < 0).sum() >= 20


@SIZES
def test_static_and_dense_lists(oracle, size):
    for seed in SEEDS:
        raw, flow, mask, kps = hostile.frame(seed, size[0], size[1], N_KP)
        depth = track_np.depth_prescale(raw, 0, 1.0, 1.0, 1.0)
        for n in (0, 1, 1023, 1024, 1025, 2048, N_KP):
            assert all_bits(track_np.static_candidates(kps[:n], depth, flow, mask, TH_BG), oracle.static_candidates(kps[:n], depth, flow, mask, TH_BG)), n
        for step in (4, 5, 8):
            a, b = track_np.dense_object_samples(depth, flow, mask, TH_OBJ, step), oracle.dense_object_samples(depth, flow, mask, TH_OBJ, step=step)
            assert all_bits(a, b) and len(a[0]) >= 20, step


def border_points(w, h, seed=3, n=600):
    """points inside, on every border, at negative fractions in (-1, 0) (they truncate to 0: inside), at w and h, and far outside"""
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    xs = [0, 0.5, 1, 1.25, -0.25, -0.999, -1, -1.5, w - 2, w - 1.5, w - 1, w - 0.5, w, w + 0.5, -1e6, 1e6]
    ys = [0, 0.5, 1, 1.25, -0.25, -0.999, -1, -1.5, h - 2, h - 1.5, h - 1, h - 0.5, h, h + 0.5, -1e6, 1e6]
    grid = np.array([(x, y) for x in xs for y in ys])
    return np.concatenate([p, grid]).astype(np.float32)


@SIZES
def test_gathers(oracle, size):
    w, h = size
    raw, flow, mask, kps = hostile.frame(SEEDS[0], w, h, N_KP)
    depth = track_np.depth_prescale(raw, 0, 1.0, 1.0, 1.0)
    corr = track_np.dense_object_samples(depth, flow, mask, TH_OBJ)[1]
    keys = np.concatenate([corr, track_np.static_candidates(kps, depth, flow, mask, TH_BG)[1], border_points(w, h)])
    assert bits(track_np.gather_static_depth(keys, depth), oracle.gather_static_depth(keys, depth))
    assert all_bits(track_np.gather_object_depth_label(keys, depth, mask, TH_OBJ), oracle.gather_object_depth_label(keys, depth, mask, TH_OBJ))


@SIZES
def test_point_samples_rule(size):
    """THE SPECIFICATION of vido_gather_point_samples: a point whose position, truncated towards zero, lies inside [0,w) x [0,h) gives the mask, depth and
    flow values of that pixel; every other point gives zeros.  So (-0.25, 3) reads pixel (0, 3); (w, 3) and (-1, 3) read nothing."""
    w, h = size
    raw, flow, mask, _ = hostile.frame(SEEDS[1], w, h, N_KP)
    pts = border_points(w, h)
    m, d, f = track_np.point_samples(pts, raw, flow, mask)
    n_in = 0
    for i, (x, y) in enumerate(pts):
        u, v = int(x), int(y)                      # Python's int() truncates towards zero like C's conversion
        if 0 <= u < w and 0 <= v < h:
            n_in += 1
            assert m[i] == mask[v, u] and bits(d[i], raw[v, u]) and bits(f[i], flow[v, u])
        else:
            assert m[i] == 0 and d[i] == 0 and (f[i] == 0).all()
    assert 100 < n_in < len(pts) - 100
    i = np.nonzero((pts[:, 0] == -0.25) & (pts[:, 1] == 1.25))[0][0]
    assert m[i] == mask[1, 0] and bits(d[i], raw[1, 0])


@SIZES
def test_update_mask_sequential_rule(oracle, size):
    w, h = size
    s = hostile.um_sequential_scene(w, h)
    _, corr, _, lab, _ = track_np.dense_object_samples(s["depth"], s["flow_last"], s["mask_last"], TH_OBJ)
    assert all_bits((corr, lab), oracle.dense_object_samples(s["depth"], s["flow_last"], s["mask_last"], TH_OBJ)[1:4:2])
    assert [int((lab == k).sum()) for k in (1, 2, 3, 4, 5)] == [144] * 5
    m_np, r_np = track_np.update_mask(lab, corr, s["mask_last"], s["flow_last"], s["mask_cur"])
    m_or, r_or = oracle.update_mask(lab, corr, s["mask_last"], s["flow_last"], s["mask_cur"])
    assert list(r_np) == list(r_or) == [1, 3] and bits(m_np, m_or)
    assert set(np.unique(m_np)) == {0, 1, 3, 4}
    # the scene is only a test of the sequential rule if a vote on the UNPATCHED mask answers differently: each label on its own against the detector's mask
    alone = [k for k in (1, 2, 3, 4, 5) if len(track_np.update_mask(lab[lab == k], corr[lab == k], s["mask_last"], s["flow_last"], s["mask_cur"])[1])]
    assert alone == [1, 2, 3, 5]


@SIZES
def test_update_mask_edges(oracle, size):
    w, h = size
    s = hostile.um_edge_scene(w, h)
    m_np, r_np = track_np.update_mask(s["last_label"], s["last_corr"], s["mask_last"], s["flow_last"], s["mask_cur"])
    m_or, r_or = oracle.update_mask(s["last_label"], s["last_corr"], s["mask_last"], s["flow_last"], s["mask_cur"])
    assert list(r_np) == list(r_or) == [7, 9, 10, 11] and bits(m_np, m_or)
    assert (m_np[h - 1, w - 18:] == 10).all() and (m_np[h - 18:, w - 1] == 10).all()            # scatter targets ON the last row / column
    assert (m_np[0, :] == 0).all() and (m_np[:, 0] == 0).all() and (m_np[1, 1:18] == 11).all() and (m_np[1:18, 1] == 11).all()      # 0 is refused, 1 is written
    assert not (m_np == 8).any()


@pytest.mark.parametrize("n", [1, 257, 1000, 4099])
def test_unproject_and_scene_flow(oracle, n):
    s = hostile.points_scene(n, n, 1242, 375)
    fx, fy, cx, cy = 718.856, 718.856, 607.1928, 185.2157
    xw = track_np.unproject_world(s["keys"], s["z"], fx, fy, cx, cy, s["Tcw"])
    assert bits(xw, oracle.unproject_world(s["keys"], s["z"], fx, fy, cx, cy, s["Tcw"]))
    assert not np.isnan(xw).any() and (xw[~(s["z"] > 0)] == 0).all()
    if n > 1:
        assert np.abs(xw).max() > 5e3                                           # the 1e4 translation is in the result: float64 accumulation of twl matters
    xc = track_np.unproject_world(s["keys"] + np.float32(1.5), np.abs(s["z"]), fx, fy, cx, cy, np.eye(4, dtype=np.float32))
    a, b = track_np.scene_flow(xw, xc, s["sem_last"], s["sem_cur"], s["obj_label"]), oracle.scene_flow(xw, xc, s["sem_last"], s["sem_cur"], s["obj_label"])
    assert all_bits(a, b)
    bad = (s["sem_last"] <= 0) | (s["sem_cur"] <= 0)
    assert (a[1][bad] == -1).all() and (a[1][~bad] == s["obj_label"][~bad]).all()
