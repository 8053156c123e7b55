"""CPU: the statement of vido_stereo_sgm (tests/refimpl/stereo_sgm_np.py) — the vectorised form against the rule read literally pixel by pixel, the bounds the rule
states (L <= 64 + p2, S <= 8 (64 + p2), |off| <= 8), its quality against synth.Scene3D.stereo_frame's exact disparity, and NetNodes' depth_source argument checks (they
come before anything is built, so they need no GPU).  The kernel is bound to the statement by equality (tests/test_stereo_sgm_gpu.py); the bars here bind the statement.

The quality bars are the issue's: of the pixels whose true disparity is below D - 1 and that lie at least 4 columns right of where their counterpart enters the right
image, at least 0.95 have status 0, and at least 0.98 of those are within 1 px of the truth."""
import numpy as np
import pytest

from refimpl import stereo_sgm_np as G
from refimpl.stereo_cases import warped_pair as _warped_pair


def test_statement_equals_the_literal_loops():
    left, right = _warped_pair(24, 18, 16, seed=1)
    for kw in (dict(max_disp=16), dict(max_disp=16, p1=3, p2=40, uniqueness=0, lr_tol=0), dict(max_disp=16, p1=1000, p2=1000, uniqueness=99, lr_tol=255)):
        want = G.stereo_sgm_loops(left, right, **kw)
        got = G.stereo_sgm(left, right, **kw)
        S = G.volumes(left, right, kw["max_disp"], kw.get("p1", 10), kw.get("p2", 120))[2]
        assert np.array_equal(S, want[4])
        for g, w_, name in zip(got, want, ("disp", "q4", "status", "stats")):
            assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g, w_), (kw, name)
    assert len(set(G.stereo_sgm(left, right, max_disp=16)[2].ravel().tolist())) >= 3             # the pair shows more than one status


def test_colour_goes_through_the_grey_rule():
    rng = np.random.RandomState(2)
    c0 = rng.randint(0, 256, (18, 24, 3)).astype(np.uint8); c1 = np.roll(c0, -3, axis=1)
    for order in (0, 1):
        want = G.stereo_sgm(G.grey(c0, order).astype(np.uint8), G.grey(c1, order).astype(np.uint8), max_disp=16)
        for g, w_ in zip(G.stereo_sgm(c0, c1, max_disp=16, rgb_order=order), want):
            assert np.array_equal(g, w_)
        for g, w_ in zip(G.stereo_sgm_loops(c0, c1, max_disp=16, rgb_order=order)[:4], want):
            assert np.array_equal(g, w_)


def test_bounds_at_the_largest_penalties():
    rng = np.random.RandomState(3)
    left, right = rng.randint(0, 256, (20, 40)).astype(np.uint8), rng.randint(0, 256, (20, 40)).astype(np.uint8)
    for l_, r_ in ((left, right), _warped_pair(40, 20, 32, seed=4)):
        C, Ls, S = G.volumes(l_, r_, 32, 1000, 1000)
        assert C.min() >= 0 and C.max() <= 64
        assert all(L.min() >= 0 and L.max() <= 64 + 1000 for L in Ls) and max(L.max() for L in Ls) > 64
        assert S.max() <= 8 * (64 + 1000) and S.max() < 1 << 16
        disp, q4, status, stats = G.select(S, 10, 1)
        d0 = S.argmin(2)
        assert np.abs(q4 - 16 * d0).max() <= 8 and stats.sum() == 20 * 40
        assert np.array_equal(disp[status == 0], q4[status == 0] / 16.0) and (disp[status != 0] == -1).all()


def test_refusals():
    img = np.zeros((16, 16), np.uint8)
    for kw in (dict(max_disp=0), dict(max_disp=24), dict(max_disp=272), dict(p1=11, p2=10), dict(p2=1001), dict(p1=-1), dict(uniqueness=100), dict(uniqueness=-1),
               dict(lr_tol=256), dict(lr_tol=-1)):
        with pytest.raises(ValueError):
            G.stereo_sgm(img, img, **{**dict(max_disp=16), **kw})
    with pytest.raises(ValueError):
        G.stereo_sgm(np.zeros((15, 16), np.uint8), np.zeros((15, 16), np.uint8), max_disp=16)
    with pytest.raises(ValueError):
        G.stereo_sgm(np.zeros((2048, 2048), np.uint8), np.zeros((2048, 2048), np.uint8), max_disp=128)      # 2^29 cells


def test_quality_on_a_scene3d_pair(vido):
    D = 64
    scene = vido.synth.Scene3D(n_frames=3, w=320, h=240, K=(250, 250, 159.5, 119.5), seed=3, objects=((-2.0, 0.2, 9.0, 0.25, 0.0, 0.05),))
    left, right, depth, mask = scene.stereo_frame(1, 0.3)
    assert np.array_equal(left, scene.frame(1)[0]) and np.array_equal(depth, scene.frame(1)[1]) and not np.array_equal(left, right)
    true = 250.0 * 0.3 / depth.astype(np.float64)
    disp, q4, status, stats = G.stereo_sgm(left, right, max_disp=D)
    pop = (true < D - 1) & (np.arange(320)[None, :] - true >= 4)
    valid = pop & (status == 0)
    share_valid = valid.sum() / pop.sum()
    share_close = (np.abs(disp[valid] - true[valid]) <= 1.0).mean()
    print("Scene3D 320 x 240, baseline 0.3, D = 64: population %d of %d, status 0 %.4f, within 1 px %.4f, stats %s, median |error| %.3f px" % (
        pop.sum(), pop.size, share_valid, share_close, stats.tolist(), np.median(np.abs(disp[valid] - true[valid]))))
    assert pop.mean() > 0.8 and mask.any()
    assert share_valid >= 0.95
    assert share_close >= 0.98


def test_netnodes_depth_source_argument_checks():
    """Refused before any network is built (no GPU needed: the checks come first)."""
    from vido_slam_amd import pipeline
    for bad in ("sgm", "STEREO", None, 1, ""):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, depth_source=bad)
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, depth_source="net", stereo_params=dict(max_disp=64))
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, depth_source="stereo", stereo_params=dict(min_disp=4))
    with pytest.raises(ValueError):
        pipeline.NetNodes(None, 480, 640, depth_source="stereo", stereo_params=[64])
    assert pipeline.NetNodes._check_depth_source("stereo", dict(max_disp=64, p1=8)) == ("stereo", dict(max_disp=64, p1=8))
    assert pipeline.NetNodes._check_depth_source("net", None) == ("net", {})
