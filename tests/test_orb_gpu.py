"""GPU parity: HIP ORB front-end (through the C-ABI) vs the CPU oracle, bit-exact at every stage.
Oracle = restatement of vido_slam/src/ORBextractor.cc (see oracle/orb_oracle.c)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=640, height=480, max_batch=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(vido):
    from vido_slam_amd import synth
    return synth.make_batch(4, 640, 480, seed=11)


def test_pyramid_fast_blur_bit_exact(ctx, frames, oracle):
    p = oracle.orb_params()
    kps, desc, cnt = ctx.orb_extract_batch(frames)
    for f in (0, 3):
        levels = oracle.orb_pyramid(p, frames[f])
        for l in range(8):
            got = ctx.orb_level(f, l)
            assert got.shape == levels[l].shape
            assert np.array_equal(got, levels[l]), (f, l)
            assert np.array_equal(ctx.orb_level(f, l, blurred=True), oracle.gaussian_blur7(levels[l])), (f, l)
            cx, cy, cr = oracle.level_candidates(p, levels[l])
            gx, gy, gs = ctx.orb_candidates(f, l)
            assert len(gx) == len(cx), (f, l, len(gx), len(cx))
            assert np.array_equal(gx - 16, cx.astype(np.int32)) and np.array_equal(gy - 16, cy.astype(np.int32)), (f, l)
            assert np.array_equal(gs, cr.astype(np.int32)), (f, l)


def test_keypoints_and_descriptors_bit_exact(ctx, frames, oracle):
    p = oracle.orb_params()
    kps, desc, cnt = ctx.orb_extract_batch(frames)
    for f in range(len(frames)):
        rk, rd, _ = oracle.orb_extract(p, frames[f])
        assert cnt[f] == len(rk)
        k = kps[f, :cnt[f]]
        for name in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(k[name], rk[name]), (f, name)
        assert np.array_equal(desc[f, :cnt[f]], rd), f


def test_single_frame_entry_matches_batch(ctx, frames):
    k1, d1 = ctx.orb_extract(frames[2])
    kps, desc, cnt = ctx.orb_extract_batch(frames)
    assert len(k1) == cnt[2]
    assert np.array_equal(k1, kps[2, :cnt[2]]) and np.array_equal(d1, desc[2, :cnt[2]])


@pytest.mark.parametrize("size", [(752, 480), (320, 240), (1241, 376)])
def test_other_frame_sizes(vido, oracle, size):
    from vido_slam_amd import synth
    w, h = size
    g = synth.make_frame(w, h, seed=5)
    c = vido.Context(width=w, height=h, max_batch=1, n_features=2500)
    k, d = c.orb_extract(g)
    p = oracle.orb_params(n_features=2500)
    rk, rd, _ = oracle.orb_extract(p, g)
    assert len(k) == len(rk)
    for name in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(k[name], rk[name]), name
    assert np.array_equal(d, rd)
    c.close()


def test_flat_and_noise_images(vido, oracle):
    c = vido.Context(width=640, height=480, max_batch=1)
    flat = np.full((480, 640), 77, np.uint8)
    k, d = c.orb_extract(flat)
    assert len(k) == 0
    rng = np.random.RandomState(0)
    noise = rng.randint(0, 256, size=(480, 640)).astype(np.uint8)     # worst case: corners everywhere
    # cv::FAST has no capacity limit (ORBextractor.cc:771-816 grows vToDistributeKeys without bound): neither has the build — every cell has as many
    # output slots as a 3x3 NMS can leave survivors, the strip kernel re-chunks its lists, the candidate buffers hold a full level
    p = oracle.orb_params()
    k, d = c.orb_extract(noise)
    rk, rd, ncand = oracle.orb_extract(p, noise)
    assert sum(ncand) > 60000                                         # far beyond round 1's 128-per-cell / 49152-per-frame limits
    assert len(k) == len(rk)
    for name in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(k[name], rk[name]), name
    assert np.array_equal(d, rd)
    for l in range(8):                                                # candidate lists (order included) per level
        x, y, s = c.orb_candidates(0, l)
        assert len(x) == ncand[l], (l, len(x), ncand[l])
    # 2x2-pixel checkerboard blocks + salt noise: equal-score plateaus (NMS ties) and cells whose 20-threshold pass comes back empty next to busy ones
    img = (np.kron(rng.randint(0, 2, size=(120, 160)) * 40 + 100, np.ones((4, 4))) + rng.randint(0, 6, size=(480, 640))).astype(np.uint8)
    img[200:, :] = 90; img[200:, :] += (rng.rand(280, 640) < 0.002).astype(np.uint8) * 15      # nearly flat lower part: the 7-threshold fallback decides there
    k, d = c.orb_extract(img)
    rk, rd, ncand = oracle.orb_extract(p, img)
    assert len(k) == len(rk)
    for name in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(k[name], rk[name]), name
    assert np.array_equal(d, rd)
    c.close()


def test_hamming_matches_oracle(ctx, oracle):
    rng = np.random.RandomState(1)
    for na, nb in ((1, 1), (7, 300), (256, 256), (2000, 2011), (33, 64)):
        a = rng.randint(0, 256, size=(na, 32)).astype(np.uint8)
        b = rng.randint(0, 256, size=(nb, 32)).astype(np.uint8)
        b[nb // 2] = a[0]; 
        if nb > 3: b[3] = b[1]                 # duplicate -> tie must resolve to the lower index
        idx, dist = ctx.hamming_match(a, b)
        ri, rd = oracle.hamming_match(a, b)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd), (na, nb)
    idx, dist = ctx.hamming_match(np.zeros((5, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert (idx == -1).all() and (dist == -1).all()


@pytest.mark.parametrize("nf,scale,levels,ini,mn", [(300, 1.2, 8, 20, 7), (1000, 1.2, 8, 20, 7), (2500, 1.2, 8, 20, 7), (1500, 1.5, 4, 20, 7),
                                                    (800, 1.2, 5, 30, 10), (4000, 1.1, 8, 12, 5)])
def test_extractor_parameter_sweep(vido, oracle, nf, scale, levels, ini, mn):
    """The device quadtree (node-list passes, final sorted passes with the early stop, best-response selection) and the rest of the
    extractor across feature budgets / pyramids / thresholds, on textured, low-texture and duplicate-heavy images: every keypoint field
    and every descriptor bit must equal the oracle's."""
    from vido_slam_amd import synth
    w, h = 640, 480
    imgs = [synth.make_frame(w, h, seed=11), synth.make_canvas(h, w, seed=12, n_rect=15),
            np.kron(synth.make_canvas(h // 4, w // 4, seed=13, n_rect=40), np.ones((4, 4), np.uint8))]       # 4x4 replicated blocks: many equal responses
    c = vido.Context(width=w, height=h, max_batch=len(imgs), n_features=nf, scale_factor=scale, n_levels=levels, ini_th_fast=ini, min_th_fast=mn)
    kps, desc, cnt = c.orb_extract_batch(np.stack(imgs))
    p = oracle.orb_params(n_features=nf, scale_factor=scale, n_levels=levels, ini_th=ini, min_th=mn)
    for f, g in enumerate(imgs):
        rk, rd, _ = oracle.orb_extract(p, g)
        assert cnt[f] == len(rk), (f, cnt[f], len(rk))
        k = kps[f, :cnt[f]]
        for name in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(k[name], rk[name]), (f, name)
        assert np.array_equal(desc[f, :cnt[f]], rd)
    c.close()


@pytest.mark.parametrize("scale,levels,last", [(1.1, 9, (149, 112)), (1.05, 16, (154, 115))])
def test_more_than_eight_levels_take_the_per_level_resize(vido, oracle, scale, levels, last):
    """A pyramid of more than 8 levels is not built by the one-launch tile kernel (it holds at most 8 levels in LDS): every level is resized from the one
    before it by a launch of its own (k_resize).  Both the lean single-frame path and the event-timed batched path run that chain; pyramid, blur, keypoints and
    descriptors must equal the oracle's bit for bit, and the single-frame result must equal frame 0 of the batch."""
    from vido_slam_amd import synth
    w, h, nfr = 320, 240, 3
    imgs = np.stack([synth.make_frame(w, h, seed=21 + f) for f in range(nfr)])
    c = vido.Context(width=w, height=h, max_batch=nfr, n_features=1000, scale_factor=scale, n_levels=levels)
    p = oracle.orb_params(n_features=1000, scale_factor=scale, n_levels=levels)
    ref_levels = [oracle.orb_pyramid(p, g) for g in imgs]
    assert len(ref_levels[0]) == levels and ref_levels[0][-1].shape == (last[1], last[0])
    ref = [oracle.orb_extract(p, g) for g in imgs]

    def check_levels(f):
        for l in range(levels):
            got = c.orb_level(f, l)
            assert got.shape == ref_levels[f][l].shape, (f, l)
            assert np.array_equal(got, ref_levels[f][l]), (f, l)
            assert np.array_equal(c.orb_level(f, l, blurred=True), oracle.gaussian_blur7(ref_levels[f][l])), (f, l)

    def check_result(f, k, d):
        rk, rd, _ = ref[f]
        assert len(k) == len(rk) and len(rk) > 0, (f, len(k), len(rk))
        for name in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(k[name], rk[name]), (f, name)
        assert np.array_equal(d, rd), f

    k1, d1 = c.orb_extract(imgs[0])                                   # one frame: lean, no stage events
    check_levels(0)
    check_result(0, k1, d1)
    kps, desc, cnt = c.orb_extract_batch(imgs)                        # three frames: the batched form
    for f in range(nfr):
        check_levels(f)
        check_result(f, kps[f, :cnt[f]], desc[f, :cnt[f]])
    assert len(k1) == cnt[0]
    assert np.array_equal(k1, kps[0, :cnt[0]]) and np.array_equal(d1, desc[0, :cnt[0]])
    c.close()
