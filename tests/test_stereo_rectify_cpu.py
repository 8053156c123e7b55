"""CPU: the statement of vido_rectify_map / vido_rectify (tests/refimpl/stereo_rectify_np.py) — the vectorised form against the rule read literally pixel by pixel;
vido_rectify_map (host code of the library, no GPU call) against the statement's map, EXACTLY; the identity and half-pixel cases; the round trip of the map through
independent code (vido_undistort_points, pinned to OpenCV's five-iteration inverse, then R, then P); and the rig test: a raw pair rendered by
synth.Scene3D.raw_stereo_frame, rectified by the statement, gives the SGM statement usable depth, and the raw pair does not.  The kernel is bound to the statement by
equality (tests/test_stereo_rectify_gpu.py); the bars here bind the statement.

Round-trip bound 0.01 px: the map's quantisation is at most (sqrt 2 / 512) x local magnification, about 0.003 px, and the five-iteration residual at these coefficients
(contraction <= 0.15 per round) about 0.002 px.  Rig bars (the issue's): of the left-inside pixels with true disparity in [1, 63), at least 0.75 valid and within 1 px on
the rectified pair, at most 0.10 on the raw pair; both maps mark at least 0.85 of the pixels inside."""
import numpy as np
import pytest

from refimpl import stereo_rectify_np as G
from refimpl import stereo_rectify_cases as CASES
from refimpl import stereo_sgm_np as SGM


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        assert False, (what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_statement_equals_the_literal_loops():
    for which in CASES.RIGS:
        cal = CASES.rig(40, 30, which)
        m, ins = G.rectify_map(src_size=(40, 30), dst_size=(37, 23), **cal)
        ml, insl = G.rectify_map_loops(src_size=(40, 30), dst_size=(37, 23), **cal)
        _same(m, ml, which); _same(ins, insl, which)
        assert 0 < ins.sum() < ins.size, which                                              # both branches of `inside`
    for deg in (120.0, 80.0):
        mb, insb = G.rectify_map(src_size=(40, 30), dst_size=(40, 30), **CASES.behind_rig(40, 30, deg))
        mbl, insbl = G.rectify_map_loops(src_size=(40, 30), dst_size=(40, 30), **CASES.behind_rig(40, 30, deg))
        _same(mb, mbl, ("behind", deg)); _same(insb, insbl, ("behind", deg))
        assert (mb == G.NO_SOURCE).any() and ((mb != G.NO_SOURCE).any() or deg == 120.0)
    for cn in (1, 3, 4):
        src = CASES.image(23, 18, cn, 5 + cn)
        for name, m in (("smooth", CASES.smooth_map(23, 18, 37, 16, 1)), ("hostile", CASES.hostile_map(23, 18, 37, 16, 2)[0]), ("planted", CASES.planted_map(23, 18, 37, 16)[0]),
                        ("rig", G.rectify_map(src_size=(23, 18), dst_size=(37, 16), **CASES.rig(23, 18))[0])):
            out, ins = G.rectify(src, m)
            outl, insl = G.rectify_loops(src, m)
            _same(out, outl, (name, cn)); _same(ins, insl, (name, cn))
            assert (out[ins == 0] == 0).all()
    census = CASES.hostile_map(23, 18, 37, 16, 2)[1]
    assert all(v > 0 for v in census.values()), census


def test_library_map_equals_the_statement_exactly(vido):
    """vido_rectify_map is host code: it runs here.  Three rigs at 64 x 48, one at 640 x 480, the sentinel branch, another destination size."""
    shown = []
    for which, sw, sh, dw, dh in [(r, 64, 48, 64, 48) for r in CASES.RIGS] + [("left", 640, 480, 640, 480), ("strong", 64, 48, 53, 41), ("right", 48, 64, 80, 70)]:
        cal = CASES.rig(sw, sh, which)
        want, wins = G.rectify_map(src_size=(sw, sh), dst_size=(dw, dh), **cal)
        got, gins = vido.rectify_map(src_size=(sw, sh), dst_size=(dw, dh), **cal)
        _same(got, want, (which, sw, sh)); _same(gins, wins, (which, sw, sh))
        shown.append((which, sw, sh, float(wins.mean())))
    print("inside shares:", shown)
    for deg in (120.0, 80.0):
        cal = CASES.behind_rig(64, 48, deg)
        want, wins = G.rectify_map(src_size=(64, 48), dst_size=(64, 48), **cal)
        got, gins = vido.rectify_map(src_size=(64, 48), dst_size=(64, 48), **cal)
        _same(got, want, ("behind", deg)); _same(gins, wins, ("behind", deg))
        n_none = int((want[..., 0] == G.NO_SOURCE).sum())
        assert (n_none == 64 * 48 if deg == 120.0 else 0 < n_none < 64 * 48) and ((want[..., 0] == G.NO_SOURCE) == (want[..., 1] == G.NO_SOURCE)).all()
    # a distortion that blows up: the polynomial leaves every range -> not finite or beyond 2^30 -> the sentinel, never a wrapped integer
    wild = dict(CASES.rig(64, 48), dist=(1e300, 1e300, 0.0, 0.0, 1e300))
    want, _ = G.rectify_map(src_size=(64, 48), dst_size=(64, 48), **wild)
    got, _ = vido.rectify_map(src_size=(64, 48), dst_size=(64, 48), **wild)
    _same(got, want, "wild")
    assert (want == G.NO_SOURCE).mean() > 0.9


def test_library_map_refusals(vido):
    import ctypes as C
    lib = vido.load_library()
    cal = CASES.rig(64, 48)
    K, d, R, P = (np.ascontiguousarray(cal[k], np.float64).ravel() for k in ("K", "dist", "R", "P"))
    m = np.full((48, 64, 2), 77, np.int32); ins = np.full((48, 64), 77, np.uint8); cnt = C.c_int32(77)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    def call(K=K, d=d, R=R, P=P, sizes=(64, 48, 64, 48), out=m):
        return lib.vido_rectify_map(None if K is None else p(K), None if d is None else p(d), None if R is None else p(R), None if P is None else p(P), *sizes,
                                    None if out is None else p(out), p(ins), C.byref(cnt))
    for kw in (dict(K=None), dict(d=None), dict(R=None), dict(P=None), dict(out=None), dict(sizes=(15, 48, 64, 48)), dict(sizes=(64, 4096, 64, 48)), dict(sizes=(64, 48, 15, 48)),
               dict(sizes=(64, 48, 64, 4096)), dict(sizes=(64, 48, 64, -1))):
        assert call(**kw) == -1, kw
    for i in range(4):
        for bad in (np.nan, np.inf):
            K2 = K.copy(); K2[i] = bad; assert call(K=K2) == -1
            P2 = P.copy(); P2[i] = bad; assert call(P=P2) == -1
    for i in range(2):
        for bad in (0.0, -1.0):
            K2 = K.copy(); K2[i] = bad; assert call(K=K2) == -1
            P2 = P.copy(); P2[i] = bad; assert call(P=P2) == -1
    d2 = d.copy(); d2[4] = np.nan; assert call(d=d2) == -1
    R2 = R.copy(); R2[8] = -np.inf; assert call(R=R2) == -1
    assert (m == 77).all() and (ins == 77).all() and cnt.value == 77                         # nothing was written by a refused call
    assert call() == 0 and cnt.value == int(ins.sum()) and cnt.value == int(G.inside_of(m, 64, 48).sum())
    lib.vido_rectify_map(p(K), p(d), p(R), p(P), 64, 48, 64, 48, p(m), None, None)           # both optional outputs absent
    with pytest.raises(vido.VidoError):
        vido.rectify_map(cal["K"], cal["dist"], cal["R"], cal["P"], (64, 48), (64, 5000))
    with pytest.raises(vido.VidoError):
        vido.rectify_map((0.0, 50.0, 1.0, 1.0), cal["dist"], cal["R"], cal["P"], (64, 48), (64, 48))


def test_identity_case():
    K = (50.0, 52.0, 31.5, 23.5)
    m, ins = G.rectify_map(K, (0, 0, 0, 0, 0), np.eye(3), K, (64, 48), (64, 48))
    u, v = np.meshgrid(np.arange(64), np.arange(48))
    assert np.array_equal(m[..., 0], 256 * u) and np.array_equal(m[..., 1], 256 * v) and ins.all()
    for cn in (1, 3, 4):
        src = CASES.image(64, 48, cn, 11)
        out, ins = G.rectify(src, m)
        assert np.array_equal(out, src) and ins.all()


def test_half_pixel_case():
    K = (50.0, 50.0, 31.5, 23.5)
    src = CASES.image(64, 48, 3, 12).astype(np.int64)
    # the rectified principal point half a pixel to the left: rectified u shows raw u + 0.5 -> the rounded mean of two columns; the last column lies outside
    m, ins = G.rectify_map(K, (0, 0, 0, 0, 0), np.eye(3), (50.0, 50.0, 31.0, 23.5), (64, 48), (64, 48))
    assert (m[..., 0] == 256 * np.arange(64)[None, :] + 128).all() and ins[:, :63].all() and not ins[:, 63].any()
    out, _ = G.rectify(src.astype(np.uint8), m)
    assert np.array_equal(out[:, :63], (src[:, :63] + src[:, 1:] + 1) >> 1) and not out[:, 63].any()
    m, ins = G.rectify_map(K, (0, 0, 0, 0, 0), np.eye(3), (50.0, 50.0, 31.5, 23.0), (64, 48), (64, 48))
    out, _ = G.rectify(src.astype(np.uint8), m)
    assert np.array_equal(out[:47], (src[:47] + src[1:] + 1) >> 1) and not out[47].any() and not ins[47].any()
    # both: the rounded mean of four
    m, _ = G.rectify_map(K, (0, 0, 0, 0, 0), np.eye(3), (50.0, 50.0, 31.0, 23.0), (64, 48), (64, 48))
    out, _ = G.rectify(src.astype(np.uint8), m)
    assert np.array_equal(out[:47, :63], (src[:47, :63] + src[:47, 1:] + src[1:, :63] + src[1:, 1:] + 2) >> 2)


@pytest.mark.parametrize("which", CASES.RIGS)
def test_round_trip_through_independent_code(vido, which):
    """map / 256 is a raw pixel; vido_undistort_points takes it to the raw camera's undistorted pixel (five iterations of the inverse, written from OpenCV's code, sharing
    nothing with the map); R and P take that back to the rectified pixel it came from."""
    w, h = 320, 240
    cal = CASES.rig(w, h, which)
    m, ins = G.rectify_map(src_size=(w, h), dst_size=(w, h), **cal)
    ok = ins.astype(bool)
    assert ok.mean() > 0.7
    raw = m[ok].astype(np.float64) / 256.0
    und = vido.undistort_points(raw.astype(np.float32), cal["K"], cal["dist"]).astype(np.float64)
    fx, fy, cx, cy = cal["K"]
    n = np.stack([(und[:, 0] - cx) / fx, (und[:, 1] - cy) / fy, np.ones(len(und))], -1) @ np.asarray(cal["R"]).T
    fxp, fyp, cxp, cyp = cal["P"]
    back = np.stack([n[:, 0] / n[:, 2] * fxp + cxp, n[:, 1] / n[:, 2] * fyp + cyp], -1)
    v, u = np.nonzero(ok)
    err = np.hypot(back[:, 0] - u, back[:, 1] - v)
    print("round trip %s: %d inside pixels, max %.5f px, mean %.5f px" % (which, len(err), err.max(), err.mean()))
    assert err.max() <= 0.01


def test_netnodes_rectify_argument_checks():
    """Refused before any network is built (no GPU needed: the checks come first)."""
    from vido_slam_amd import pipeline
    cal = dict(K=(500.0, 500.0, 319.5, 239.5), dist=CASES.KAIST_DIST, R=CASES.R_LEFT, P=(470.0, 470.0, 319.5, 239.5))
    for kw in (dict(rectify=dict(left=cal, right=cal)), dict(rectify=dict(left=cal), depth_source="stereo"), dict(rectify=dict(left=cal, centre=cal)),
               dict(rectify=dict(right=cal), depth_source="stereo"), dict(rectify=dict(left=dict(cal, k4=0.0))), dict(rectify=dict(left=dict(cal, P=(470.0, -1.0, 319.5, 239.5)))),
               dict(rectify=dict(left=cal, raw_size=(8, 640))), dict(rectify=(cal, cal), depth_source="stereo")):
        with pytest.raises(ValueError):
            pipeline.NetNodes(None, 480, 640, **kw)
    assert pipeline.NetNodes._check_rectify(None, "net", 480, 640) is None
    got = pipeline.NetNodes._check_rectify(dict(left=cal, right=cal, raw_size=(240, 320)), "stereo", 480, 640)
    assert got["raw_size"] == (240, 320) and got["right"]["R"].shape == (9,) and np.array_equal(got["left"]["R"], np.asarray(CASES.R_LEFT).ravel())


RIG = dict(w=320, h=240, P=(235.0, 235.0, 159.5, 119.5), K_raw=(250.0, 250.0, 159.5, 119.5), baseline=0.5, frame=1, seed=3, max_disp=64, p2=100)


def rig_measure(vido):
    """The rig test's numbers (tools/measure_stereo_rectify.py prints them too): dict(inside_left, inside_right, population, rectified, raw, direct)."""
    w, h, P, K_raw = RIG["w"], RIG["h"], RIG["P"], RIG["K_raw"]
    scene = vido.synth.Scene3D(w=w, h=h, K=P, seed=RIG["seed"])
    left, right, depth, _ = scene.stereo_frame(RIG["frame"], RIG["baseline"])
    raw_l, raw_r = scene.raw_stereo_frame(RIG["frame"], RIG["baseline"], K_raw, CASES.KAIST_DIST, CASES.R_LEFT, CASES.R_RIGHT)
    ml, il = G.rectify_map(K_raw, CASES.KAIST_DIST, CASES.R_LEFT, P, (w, h), (w, h))
    mr, ir = G.rectify_map(K_raw, CASES.KAIST_DIST, CASES.R_RIGHT, P, (w, h), (w, h))
    rect_l, _ = G.rectify(raw_l, ml); rect_r, _ = G.rectify(raw_r, mr)
    true = P[0] * RIG["baseline"] / depth.astype(np.float64)
    pop = il.astype(bool) & (true >= 1) & (true < 63)
    res = dict(inside_left=float(il.mean()), inside_right=float(ir.mean()), population=int(pop.sum()))
    for name, (a, b) in (("rectified", (rect_l, rect_r)), ("raw", (raw_l, raw_r)), ("direct", (left, right))):
        disp, _, status, _ = SGM.stereo_sgm(a, b, max_disp=RIG["max_disp"], p2=RIG["p2"])
        good = pop & (status == 0) & (np.abs(disp - true) <= 1.0)
        res[name] = float(good.sum() / pop.sum()); res[name + "_valid"] = float((pop & (status == 0)).sum() / pop.sum())
    return res


def test_rig_pair_becomes_usable_depth(vido):
    r = rig_measure(vido)
    print("rig 320 x 240: inside %.4f / %.4f, population %d; valid and within 1 px: rectified %.4f (valid %.4f), raw %.4f (valid %.4f), rendered in the rectified cameras "
          "%.4f (valid %.4f)" % (r["inside_left"], r["inside_right"], r["population"], r["rectified"], r["rectified_valid"], r["raw"], r["raw_valid"], r["direct"], r["direct_valid"]))
    assert r["inside_left"] >= 0.85 and r["inside_right"] >= 0.85
    assert r["rectified"] >= 0.75
    assert r["raw"] <= 0.10
