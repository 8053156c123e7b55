"""GPU: vido_orb_describe_points (csrc/orb.hip k_describe_points) — orientation, steered rBRIEF and Hamming distance at caller-given points of a
resident pyramid slab.  Everything here is an integer / bit pattern: no tolerance anywhere.  The reference never evaluates a descriptor away from a
keypoint, so parity is defined by the oracle's per-point vo_ic_angle / vo_brief on the build's own pyramid (vido_orb_read_level)."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = 19                                   # the extractor's edge margin (EDGE_THRESHOLD): valid points are EDGE <= x < w - EDGE, same for y
POPCNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _popcount_dist(a, b):
    return POPCNT[np.bitwise_xor(a, b)].sum(axis=1).astype(np.int32)


def _kp_xyl(kps, p):
    """Level coordinates and level of the extractor's keypoints (kp.x = level x * scale[level], float)."""
    lv = kps["octave"].astype(np.int32)
    sc = np.array([p.scale[l] for l in lv], np.float32)
    return np.stack([np.rint(kps["x"] / sc).astype(np.int32), np.rint(kps["y"] / sc).astype(np.int32), lv], 1)


def _images(synth, w, h):
    return [synth.make_frame(w, h, seed=11), synth.make_canvas(h, w, seed=12, n_rect=15),
            np.kron(synth.make_canvas(h // 4, w // 4, seed=13, n_rect=40), np.ones((4, 4), np.uint8))]


def _oracle_points(oracle, p, levels, blurred, xyl):
    """Per-point oracle results with the kernel's invalid triple outside the margin."""
    n = len(xyl)
    ang = np.full(n, -1.0, np.float32); desc = np.zeros((n, 32), np.uint8); valid = np.zeros(n, bool)
    for i, (x, y, l) in enumerate(xyl):
        if l < 0 or l >= len(levels):
            continue
        h, w = levels[l].shape
        if not (EDGE <= x < w - EDGE and EDGE <= y < h - EDGE):
            continue
        valid[i] = True
        ang[i] = oracle.ic_angle(levels[l], x, y, p)
        desc[i] = oracle.brief(blurred[l], x, y, ang[i])
    return ang, desc, valid


@pytest.mark.parametrize("size", [(640, 480), (752, 480)])
def test_own_keypoints_reproduce_the_extractor(vido, oracle, size):
    """Describing a frame's own keypoints gives the extractor's angles and descriptors bit for bit, and distance 0 to them."""
    w, h = size
    p = oracle.orb_params()
    imgs = _images(vido.synth, w, h) if size == (640, 480) else [vido.synth.make_frame(w, h, seed=5)]
    c = vido.Context(width=w, height=h, max_batch=1)
    for g in imgs:
        kps, desc = c.orb_extract(g)
        assert len(kps) > 200
        xyl = _kp_xyl(kps, p)
        ang, d, dist = c.orb_describe_points(0, xyl, desc)
        assert np.array_equal(ang, kps["angle"])
        assert np.array_equal(d, desc)
        assert np.array_equal(dist, np.zeros(len(kps), np.int32))
    c.close()


def _random_points(rng, c, kps_xyl, per_level=4000):
    pts = [kps_xyl]
    for l in range(8):
        lw, lh = c.orb_level(0, l).shape[::-1]
        r = np.stack([rng.randint(-2, lw + 2, per_level), rng.randint(-2, lh + 2, per_level), np.full(per_level, l)], 1)      # some fall outside the margin
        r[: per_level * 3 // 4, 0] = rng.randint(EDGE, lw - EDGE, per_level * 3 // 4); r[: per_level * 3 // 4, 1] = rng.randint(EDGE, lh - EDGE, per_level * 3 // 4)
        xs = [EDGE, lw - EDGE - 1, EDGE - 1, lw - EDGE, lw // 2]; ys = [EDGE, lh - EDGE - 1, EDGE - 1, lh - EDGE, lh // 2]
        edge = np.array([(x, y, l) for x in xs for y in ys])                # exactly on the valid margin, one pixel outside it, every combination
        pts += [r, edge]
    pts.append(np.array([(100, 100, -1), (100, 100, 8), (100, 100, 1 << 20), (-(1 << 30), 50, 0), (50, (1 << 30), 0)]))
    return np.concatenate(pts).astype(np.int32)


@pytest.fixture(scope="module")
def arbitrary(vido, oracle):
    p = oracle.orb_params()
    g = vido.synth.make_frame(640, 480, seed=11)
    c = vido.Context(width=640, height=480, max_batch=2)
    kps, desc, cnt = c.orb_extract_batch(np.stack([g, vido.synth.make_frame(640, 480, seed=23)]))
    rng = np.random.RandomState(5)
    xyl = _random_points(rng, c, _kp_xyl(kps[0][:cnt[0]], p))
    ref = rng.randint(0, 256, size=(len(xyl), 32)).astype(np.uint8)
    levels = [[c.orb_level(f, l) for l in range(8)] for f in range(2)]
    blurred = [[c.orb_level(f, l, blurred=True) for l in range(8)] for f in range(2)]
    yield dict(c=c, p=p, xyl=xyl, ref=ref, levels=levels, blurred=blurred, n_kp=int(cnt[0]))
    c.close()


def test_arbitrary_points_match_oracle(arbitrary, oracle):
    """>= 4000 random integer points per level over all 8 levels (most of them not keypoints), the valid margin and one pixel outside it: angle and descriptor
    equal the oracle's on the levels the context itself returns, distances equal numpy's popcount, outside points give the invalid triple."""
    A = arbitrary; c, xyl, ref = A["c"], A["xyl"], A["ref"]
    assert len(xyl) - A["n_kp"] >= 8 * 4000 and len(xyl) - A["n_kp"] >= len(xyl) // 2
    ang, desc, dist = c.orb_describe_points(0, xyl, ref)
    rang, rdesc, valid = _oracle_points(oracle, A["p"], A["levels"][0], A["blurred"][0], xyl)
    assert valid.sum() > 8 * 3000 and (~valid).sum() > 8 * 16
    assert np.array_equal(ang, rang)
    assert np.array_equal(desc, rdesc)
    rdist = np.where(valid, _popcount_dist(rdesc, ref), -1).astype(np.int32)
    assert np.array_equal(dist, rdist)
    assert np.all(dist[~valid] == -1) and np.all(ang[~valid] == -1) and not desc[~valid].any()
    a2, d2, none = c.orb_describe_points(0, xyl)                          # without reference descriptors: no distances, same rest
    assert none is None and np.array_equal(a2, ang) and np.array_equal(d2, desc)


def test_order_count_frame_and_device_form(arbitrary, oracle, vido):
    A = arbitrary; c, xyl, ref = A["c"], A["xyl"], A["ref"]
    ang, desc, dist = c.orb_describe_points(0, xyl, ref)
    ra, rd, rdi = c.orb_describe_points(0, xyl[::-1], ref[::-1])          # reversed order
    assert np.array_equal(ra[::-1], ang) and np.array_equal(rd[::-1], desc) and np.array_equal(rdi[::-1], dist)
    for i in (0, A["n_kp"] + 7, len(xyl) - 1):                            # n = 1
        a1, d1, di1 = c.orb_describe_points(0, xyl[i:i + 1], ref[i:i + 1])
        assert a1[0] == ang[i] and np.array_equal(d1[0], desc[i]) and di1[0] == dist[i]
    sub = xyl[A["n_kp"]:A["n_kp"] + 6000]; sref = ref[A["n_kp"]:A["n_kp"] + 6000]      # a frame index that is not 0
    a1, d1, di1 = c.orb_describe_points(1, sub, sref)
    rang, rdesc, valid = _oracle_points(oracle, A["p"], A["levels"][1], A["blurred"][1], sub)
    assert np.array_equal(a1, rang) and np.array_equal(d1, rdesc)
    assert np.array_equal(di1, np.where(valid, _popcount_dist(rdesc, sref), -1))
    assert not np.array_equal(d1, desc[A["n_kp"]:A["n_kp"] + 6000])       # (the two frames differ)
    # device-pointer form: enqueue only, results after a synchronize
    import torch
    n = len(xyl)
    t_xyl = torch.from_numpy(xyl.copy()).cuda(); t_ref = torch.from_numpy(ref.copy()).cuda()
    t_ang = torch.empty(n, dtype=torch.float32, device="cuda"); t_desc = torch.empty((n, 32), dtype=torch.uint8, device="cuda"); t_dist = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.orb_describe_points_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), t_ang.data_ptr(), t_desc.data_ptr(), t_dist.data_ptr())
    c.synchronize()
    assert np.array_equal(t_ang.cpu().numpy(), ang) and np.array_equal(t_desc.cpu().numpy(), desc) and np.array_equal(t_dist.cpu().numpy(), dist)
    t_dist.fill_(-7); torch.cuda.synchronize()                             # distances alone: no descriptor is written anywhere
    c.orb_describe_points_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), None, None, t_dist.data_ptr())
    c.synchronize()
    assert np.array_equal(t_dist.cpu().numpy(), dist)


def test_bad_arguments_leave_the_context_usable(arbitrary, vido):
    A = arbitrary; c, xyl, ref = A["c"], A["xyl"][:64], A["ref"][:64]
    good = c.orb_describe_points(0, xyl, ref)
    lib = c.lib
    ang = np.empty(64, np.float32); desc = np.empty((64, 32), np.uint8); dist = np.empty(64, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vido_orb_describe_points(c.h, 0, P(xyl), 0, None, None, None, None, 0) == 0               # n == 0: successful no-op
    assert lib.vido_orb_describe_points(c.h, 0, None, 0, None, P(ang), P(desc), None, 0) == 0
    for frame in (-1, 2, 1 << 20):                                                                         # the context was created for a batch of 2
        assert lib.vido_orb_describe_points(c.h, frame, P(xyl), 64, P(ref), P(ang), P(desc), P(dist), 0) == -1
    assert lib.vido_orb_describe_points(c.h, 0, P(xyl), -1, P(ref), P(ang), P(desc), P(dist), 0) == -1
    assert lib.vido_orb_describe_points(c.h, 0, None, 64, P(ref), P(ang), P(desc), P(dist), 0) == -1
    assert lib.vido_orb_describe_points(c.h, 0, P(xyl), 64, None, P(ang), P(desc), P(dist), 0) == -1       # distances without reference descriptors
    assert lib.vido_orb_describe_points(None, 0, P(xyl), 64, P(ref), P(ang), P(desc), P(dist), 0) == -1
    with pytest.raises(vido.VidoError):
        c.orb_describe_points(0, xyl, ref[:10])
    again = c.orb_describe_points(0, xyl, ref)
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
