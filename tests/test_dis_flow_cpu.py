"""CPU: properties of the statement of vido_dis_flow (tests/refimpl/dis_flow_np.py) — what follows from the definition alone, the bounds its docstring states, and its
accuracy against synth.Scene3D's exact flow.  The kernel is bound to the statement by equality (tests/test_dis_flow_gpu.py); the bars here bind the statement.

The accuracy bars are those of the float prototype the definition was drawn from (static: median 0.13 px, 0.87 under 1 px; object: median 0.10-0.12 px, 0.89-0.93 under
1 px), with twice the median and 0.07-0.09 off the shares for the details the integer form fixes differently."""
import numpy as np
import pytest

from refimpl import dis_flow_np as D
from refimpl import patch_refine_np as R


def _checker(n=64):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((((yy >> 1) + (xx >> 1)) & 1) * 255).astype(np.uint8)


def _smooth(n=64, seed=5):
    """patch_refine_np.smooth_tile enlarged to n x n: random values on a 3-px grid, bilinearly upsampled"""
    tile, R.TILE = R.TILE, n
    try:
        return R.smooth_tile(seed)
    finally:
        R.TILE = tile


def test_identical_images_give_zero_flow_and_consistent_stats(vido):
    img = vido.synth.make_frame(97, 66, seed=4)
    flow, q8, stats = D.dis_flow(img, img, coarsest=2)
    assert q8.shape == (66, 97, 2) and q8.dtype == np.int32 and flow.dtype == np.float32 and stats.dtype == np.int32
    assert not q8.any() and not flow.any()
    assert stats[:3].sum() == D.n_patches(66, 97, 2) and stats[2] == 0 and stats[3] == 0       # e = 0 everywhere: the first step is (0, 0)


def test_constant_image_is_flat_everywhere():
    img = np.full((40, 56), 93, np.uint8)
    other = np.random.RandomState(1).randint(0, 256, (40, 56)).astype(np.uint8)
    flow, q8, stats = D.dis_flow(img, other, coarsest=2)
    assert stats.tolist() == [0, D.n_patches(40, 56, 2), 0, 0] and not q8.any()


def test_constructed_checkers_reach_the_stated_bounds():
    """The 2-px checker has gx, gy = +-255 on every pixel of an interior patch, summing to 0: H = 64^2 255^2, the bound.  Against its inverse |e| = 4080 on every pixel, half
    of each sign: cost = 64^2 4080^2, the bound, while e is out of step with the gradients (b = 0).  Against the checker moved by one pixel e = +-4080 on half of the
    pixels, in step with gx: |b| = 64 * 32 * 255 * 4080, half the bound — a central difference cannot be in step with the template on every pixel, so the bound itself
    is not attainable — and |2 num| = 2 H |b| = 2^59.98.  Nothing passes a bound."""
    c = _checker()
    tr = {}
    D.dis_flow(c, (255 - c).astype(np.uint8), coarsest=0, trace=tr)
    assert tr["max_h"] == D.BOUNDS["max_h"] and tr["max_e"] == D.BOUNDS["max_e"] and tr["max_cost"] == D.BOUNDS["max_cost"]
    tr2 = {}
    D.dis_flow(c, np.roll(c, 1, axis=1), coarsest=0, iters=16, max_shift_q8=2048, trace=tr2)
    assert tr2["max_h"] == D.BOUNDS["max_h"]
    assert tr2["max_b"] == D.BOUNDS["max_b"] // 2
    assert tr2["max_2num"] == 2 * D.BOUNDS["max_h"] * (D.BOUNDS["max_b"] // 2) and tr2["max_2num"] > 1 << 59
    for t in (tr, tr2):
        for k, v in D.BOUNDS.items():
            assert t.get(k, 0) <= v, (k, t[k], v)
    assert D.BOUNDS["max_h"] < 1 << 28 and D.BOUNDS["max_b"] < 1 << 32 and D.BOUNDS["max_cost"] < 1 << 36
    assert 2 * 2 * D.BOUNDS["max_h"] * D.BOUNDS["max_b"] < D.BOUNDS["max_2num"]                 # 2 |Hyy bx - Hxy by| <= 2 * 2 H b


def test_step_equals_the_one_division_it_replaces():
    rng = np.random.RandomState(3)
    det = rng.randint(1, 1 << 56, 4000, dtype=np.int64); num = rng.randint(-(1 << 61) + 1, 1 << 61, 4000, dtype=np.int64)
    det[:2000] = rng.randint(1, 1 << 20, 2000); num[:2000] = rng.randint(-(1 << 24), 1 << 24, 2000); num[:8] = [0, 1, -1, 8, -8, 2 ** 61 - 1, -(2 ** 61) + 1, 5]
    got = D.step(num, det)
    want = [min(max(R.rdiv(-32 * int(a), int(d)), -256), 256) for a, d in zip(num, det)]
    assert got.tolist() == want


def test_unrelated_noise_finishes():
    rng = np.random.RandomState(2)
    a, b = rng.randint(0, 256, (64, 64)).astype(np.uint8), rng.randint(0, 256, (64, 64)).astype(np.uint8)
    flow, q8, stats = D.dis_flow(a, b, coarsest=2, iters=16)
    assert stats[:3].sum() == D.n_patches(64, 64, 2) and stats[2] > 0                           # rejections happen
    assert np.abs(q8).max() < 1 << 19 and np.array_equal(flow, q8.astype(np.float32) / 256)


@pytest.mark.parametrize("n,want", [(8, [0]), (9, [0, 1]), (11, [0, 3]), (12, [0, 4]), (30, [0, 4, 8, 12, 16, 20, 22])])
def test_patch_origins(n, want):
    assert D.origins(n).tolist() == want


def test_colour_form_equals_the_grey_form_of_the_converted_image(vido):
    rng = np.random.RandomState(6)
    a, b = rng.randint(0, 256, (33, 47, 3)).astype(np.uint8), rng.randint(0, 256, (33, 47, 3)).astype(np.uint8)
    for order in (0, 1):
        ga, gb = D.grey(a, order).astype(np.uint8), D.grey(b, order).astype(np.uint8)
        a64 = a.astype(np.int64)
        B, G_, Rr = (a64[..., 2], a64[..., 1], a64[..., 0]) if order else (a64[..., 0], a64[..., 1], a64[..., 2])
        assert np.array_equal(ga, (1868 * B + 9617 * G_ + 4899 * Rr + 8192) >> 14)
        want = D.dis_flow(ga, gb, coarsest=1)
        for img0, img1 in ((a, b), (np.dstack([a, a[..., :1]]), np.dstack([b, b[..., :1]]))):
            got = D.dis_flow(img0, img1, coarsest=1, rgb_order=order)
            assert all(np.array_equal(x, y) for x, y in zip(got, want))
    g = vido.synth.make_frame(40, 24, seed=2)
    assert np.array_equal(D.grey(vido.synth.gray_to_bgr(g)), g)


def test_known_shift_of_a_smooth_texture_comes_back():
    """A condition on the definition: a smooth texture resampled by the statement's own bilinear form at (+0.75, -0.5) px comes back within 1/8 px, at the median over the
    pixels at least 12 px from the border."""
    img = _smooth(64)
    dx, dy = 192, -128
    moved = D.resample(img, -dx, -dy)                                    # moved(x) = img(x - d): the content moves by +d
    flow, q8, stats = D.dis_flow(img, moved, coarsest=2)
    err = np.hypot(q8[12:-12, 12:-12, 0] - dx, q8[12:-12, 12:-12, 1] - dy) / 256.0
    print("known shift: median error %.4f px, max %.4f px, stats %s" % (np.median(err), err.max(), stats.tolist()))
    assert np.median(err) <= 0.125


def test_accuracy_against_scene3d(vido):
    sc = vido.synth.Scene3D()
    g1, _, f1, m1 = sc.frame(1); g2 = sc.frame(2)[0]
    flow, q8, stats = D.dis_flow(g1, g2, **D.DEFAULTS)
    h, w = g1.shape
    Y, X = np.mgrid[0:h, 0:w]
    tx, ty = X + f1[..., 0], Y + f1[..., 1]
    inside = (tx >= 8) & (tx <= w - 1 - 8) & (ty >= 8) & (ty <= h - 1 - 8)
    epe = np.hypot(flow[..., 0] - f1[..., 0], flow[..., 1] - f1[..., 1])
    res = {}
    for name, sel in (("static", inside & (m1 == 0)), ("object", inside & (m1 > 0))):
        e = epe[sel]; res[name] = (float(np.median(e)), float((e < 1).mean()))
        print("%s: %d pixels, median EPE %.3f px, share < 0.4 px %.3f, < 1 px %.3f, p90 %.2f px" % (name, sel.sum(), np.median(e), (e < 0.4).mean(), (e < 1).mean(), np.percentile(e, 90)))
    assert res["static"][0] <= 0.26 and res["static"][1] >= 0.78
    assert res["object"][0] <= 0.24 and res["object"][1] >= 0.82


def test_parameters_out_of_range_raise():
    img = np.zeros((32, 32), np.uint8)
    for kw in (dict(coarsest=-1), dict(coarsest=7), dict(coarsest=3), dict(iters=0), dict(iters=17), dict(max_shift_q8=-1), dict(max_shift_q8=2049), dict(min_eig=-1)):
        with pytest.raises(ValueError):
            D.dis_flow(img, img, **kw)
    with pytest.raises(ValueError):
        D.dis_flow(np.zeros((15, 32), np.uint8), np.zeros((15, 32), np.uint8), coarsest=0)
