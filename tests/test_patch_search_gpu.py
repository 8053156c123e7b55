"""MI355X: vido_orb_patch_search (csrc/patchsearch.hip k_patch_search) against the numpy / Python-integer statement (tests/refimpl/patch_search_np.py) on the level images
the context itself returns (vido_orb_read_level): dxy, sums, second, status and stats bit for bit, no tolerance anywhere.  Frames 64 x 64 (one level: a pyramid level must
be 62 px wide, so its "top level" is level 0, which the 40-px window of radius 16 leaves at every border point), 201 x 151 (odd size, 5 levels) and 1242 x 375 (8 levels);
levels 0, 3 and the top one; both planes; radius 0, 1, 3, 8, 16; excl 1, 2, radius; every border; n across the wave and the four-point workgroup edge.
Status 3 needs a candidate outside the exclusion zone, so it cannot occur at radius 0; every other case must see all five statuses."""
import ctypes as C
import numpy as np
import pytest

from refimpl import patch_points_np as PP
from refimpl import patch_search_np as R
from refimpl.patch_points_np import constructed

pytestmark = pytest.mark.gpu

SIZES = {"64x64": (64, 64, 1), "201x151": (201, 151, 5), "1242x375": (1242, 375, 8)}
RADII = (0, 1, 3, 8, 16)
MIN_VAR, MIN_Q, RATIO = 147456, 920, 900


def _points(rng, lw, lh, level, n_levels, radius, n_rand):
    """x, y in {the last value without a candidate, the first with one, the first whose own patch is inside, ...} on all four sides, random interior points, random points
    around and beyond the level, huge coordinates and levels out of range."""
    xs = [3 - radius, 4 - radius, 4, 5, 6, 7, lw - 4, lw - 4 + radius, lw - 3 + radius, lw // 2]; ys = [3 - radius, 4 - radius, 4, lh - 4, lh - 4 + radius, lh - 3 + radius, lh // 2]
    pts = [(x, y, level) for x in xs for y in ys]
    r = np.stack([rng.randint(4, lw - 3, n_rand), rng.randint(4, lh - 3, n_rand), np.full(n_rand, level)], 1)
    o = np.stack([rng.randint(-radius - 6, lw + radius + 6, n_rand // 3), rng.randint(-radius - 6, lh + radius + 6, n_rand // 3), np.full(n_rand // 3, level)], 1)
    bad = [(20, 20, -1), (20, 20, n_levels), (20, 20, 1 << 20), (-(1 << 31), 20, level), ((1 << 31) - 1, 20, level), (20, -(1 << 31), level), (20, (1 << 31) - 1, level), (-1 - radius, -1, level)]
    return np.concatenate([np.array(pts), r, o, np.array(bad, np.int64)]).astype(np.int32)


def _references(rng, levels, xyl, radius):
    """Per point, by k mod 6: (0, 1) the level's own patch at a random offset inside the window, (2) the same with noise, (3) the patch of another random place,
    (4) random bytes, (5) the constructed patches in turn (checkerboards, ramps, flat ones)."""
    cons = [v[i] for v in constructed().values() for i in (0, 1)]
    n = len(xyl); ref = np.empty((n, 64), np.uint8)
    for k, (x, y, l) in enumerate(xyl.astype(np.int64)):
        kind = k % 6
        lv = levels[l] if 0 <= l < len(levels) else levels[0]; h, w = lv.shape
        if kind in (0, 1, 2):
            sx = int(min(max(min(max(x, -99), w + 99) + rng.randint(-radius, radius + 1), 4), w - 4)); sy = int(min(max(min(max(y, -99), h + 99) + rng.randint(-radius, radius + 1), 4), h - 4))
        else:
            sx, sy = int(rng.randint(4, w - 3)), int(rng.randint(4, h - 3))
        v = lv[sy - 4:sy + 4, sx - 4:sx + 4].reshape(64).astype(np.float64)
        if kind == 2:
            v = v + rng.normal(0, 6, 64)
        elif kind == 4:
            v = rng.randint(0, 256, 64)
        elif kind == 5:
            v = cons[(k // 6) % len(cons)]
        ref[k] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return ref


@pytest.fixture(scope="module", params=list(SIZES))
def ctxs(request, vido):
    """One context per frame size, batch of 2 with two different frames extracted; the level images of both planes read back once."""
    w, h, nl = SIZES[request.param]
    c = vido.Context(width=w, height=h, max_batch=2, n_features=500, n_levels=nl)
    c.orb_extract_batch(np.stack([vido.synth.make_frame(w, h, seed=31), vido.synth.make_canvas(h, w, seed=32, n_rect=30)]))
    planes = {(f, b): [c.orb_level(f, l, blurred=bool(b)) for l in range(nl)] for f in range(2) for b in range(2)}
    yield dict(c=c, nl=nl, planes=planes, name=request.param)
    c.close()


def _inputs(A, frame, blurred, radius, seed, n_rand=90):
    rng = np.random.RandomState(seed); levels = A["planes"][frame, blurred]; nl = A["nl"]
    xyl = np.concatenate([_points(rng, levels[l].shape[1], levels[l].shape[0], l, nl, radius, n_rand) for l in sorted({0, min(3, nl - 1), nl - 1})])
    return xyl, _references(rng, levels, xyl, radius)


def _same(got, want):
    assert len(got) == len(want) == 5
    for g, w_, name in zip(got, want, ("dxy", "sums", "second", "status", "stats")):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if not np.array_equal(g, w_):
            bad = np.flatnonzero((g != w_).reshape(len(g), -1).any(1))
            assert False, (name, bad[:8], g[bad[:4]], w_[bad[:4]])


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("blurred", [0, 1])
def test_bit_equal_on_every_border_level_radius_and_excl(ctxs, blurred, radius):
    A = ctxs; c = A["c"]; levels = A["planes"][0, blurred]
    xyl, ref = _inputs(A, 0, blurred, radius, 100 + radius)
    seen = set(); n_searched = 0; n_all = 0
    for excl in sorted({1, 2, max(radius, 1)}):
        want = R.patch_search(levels, xyl, ref, radius, excl, MIN_VAR, MIN_Q, RATIO)
        _same(c.orb_patch_search(0, xyl, ref, radius, excl=excl, blurred=blurred, min_var=MIN_VAR, min_zncc_q10=MIN_Q, peak_ratio_q10=RATIO), want)
        seen |= set(want[3].tolist()); n_searched += int(np.isin(want[3], (0, 1, 3)).sum()); n_all += len(xyl)
        assert want[4].sum() == len(xyl)
    print("patch_search %s blurred %d radius %d: %d points, statuses 0 1 2 3 -1 of the last excl = %s, searched %d of %d" % (A["name"], blurred, radius, len(xyl), want[4].tolist(), n_searched, n_all))
    assert seen == ({-1, 0, 1, 2} if radius == 0 else {-1, 0, 1, 2, 3})
    assert 2 * n_searched >= n_all                                                # a kernel that declines everything cannot pass
    lw, lh = levels[0].shape[::-1]; st = want[3]
    for x, y, ok in ((4 - radius, 4 - radius, True), (lw - 4 + radius, lh - 4 + radius, True), (3 - radius, 4, False), (4, 3 - radius, False), (lw - 3 + radius, 4, False), (4, lh - 3 + radius, False)):
        i = int(np.flatnonzero((xyl[:, 0] == x) & (xyl[:, 1] == y) & (xyl[:, 2] == 0))[0])
        assert bool(st[i] >= 0) == ok


def test_thresholds_and_the_peak_test_switched_off(ctxs):
    A = ctxs; c = A["c"]; levels = A["planes"][0, 1]
    xyl, ref = _inputs(A, 0, 1, 3, 7, n_rand=24)
    for min_var, q, ratio in ((0, 0, 0), (0, 1024, 1024), (1, 512, 1), (4096, 920, 0), (66585600, 0, 512)):
        want = R.patch_search(levels, xyl, ref, 3, 1, min_var, q, ratio)
        _same(c.orb_patch_search(0, xyl, ref, 3, excl=1, min_var=min_var, min_zncc_q10=q, peak_ratio_q10=ratio), want)
        assert ratio or want[4][3] == 0


def test_n_order_single_points_and_the_second_slab(ctxs):
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A, 0, 1, 8, 5, n_rand=160)
    assert len(xyl) >= 257
    kw = dict(excl=2, min_var=4096, min_zncc_q10=920, peak_ratio_q10=RATIO)
    full = c.orb_patch_search(0, xyl, ref, 8, **kw)
    _same(full, R.patch_search(A["planes"][0, 1], xyl, ref, 8, 2, 4096, 920, RATIO))
    cnt = lambda st: np.array([(st == s).sum() for s in (0, 1, 2, 3, -1)], np.int32)
    for n in (0, 1, 3, 4, 5, 257):                                                # across the workgroup edge of four points; n == 0: empty outputs, stats zero
        got = c.orb_patch_search(0, xyl[:n], ref[:n], 8, **kw)
        _same(got, tuple(v[:n] for v in full[:4]) + (cnt(full[3][:n]),))
    rev = c.orb_patch_search(0, xyl[::-1], ref[::-1], 8, **kw)
    _same(tuple(v[::-1] for v in rev[:4]) + (rev[4],), full)
    for i in (0, 7, len(xyl) // 2, len(xyl) - 1):
        one = c.orb_patch_search(0, xyl[i:i + 1], ref[i:i + 1], 8, **kw)
        _same(one, tuple(v[i:i + 1] for v in full[:4]) + (cnt(full[3][i:i + 1]),))
    for b in (0, 1):                                                              # slab 1 of the batch of 2: the other frame, references from it
        x1, r1 = _inputs(A, 1, b, 3, 11, n_rand=24)
        got = c.orb_patch_search(1, x1, r1, 3, blurred=b, **kw)
        _same(got, R.patch_search(A["planes"][1, b], x1, r1, 3, 2, 4096, 920, RATIO))
        assert not np.array_equal(got[1], c.orb_patch_search(0, x1, r1, 3, blurred=b, **kw)[1])


def test_constructed_patches_uploaded_as_a_frame(vido):
    """The checkerboard at VAR_MAX (every comparison at its largest operands: cov^2 var 2^20 near 2^98), its inverse, and the other constructed pairs pasted into a frame
    and searched on the unblurred level 0, where the level IS the uploaded image."""
    w, h, nl = SIZES["201x151"]
    cases = constructed(); names = sorted(cases)
    yy, xx = np.mgrid[0:h, 0:w]; img = np.full((h, w), 128, np.uint8); img[:, :100] = ((((yy + xx) & 1) * 255).astype(np.uint8))[:, :100]
    xyl = [(40, 40, 0), (41, 40, 0), (41, 100, 0), (60, 75, 0)]; ref = [cases["checker"][0], cases["checker"][0], cases["checker_inverse"][1], cases["checker"][0]]
    for i, name in enumerate(names):
        x, y = 112 + 10 * i + (i & 3), 12 + 25 * (i % 5)
        img[y - 4:y + 4, x - 4:x + 4] = cases[name][1].reshape(8, 8); xyl.append((x - 1, y + 2, 0)); ref.append(cases[name][0])
    xyl = np.array(xyl, np.int32); ref = np.stack(ref)
    c = vido.Context(width=w, height=h, max_batch=1, n_features=500, n_levels=nl)
    c.orb_extract(img)
    assert np.array_equal(c.orb_level(0, 0), img)
    for radius, excl, q, ratio in ((16, 1, 1024, 1024), (16, 1, 1024, 1023), (8, 2, 920, 0), (3, 3, 0, 512), (0, 1, 512, 0)):
        for min_var in (0, 1, 147456):
            want = R.patch_search([img], xyl, ref, radius, excl, min_var, q, ratio)
            got = c.orb_patch_search(0, xyl, ref, radius, excl=excl, blurred=0, min_var=min_var, min_zncc_q10=q, peak_ratio_q10=ratio)
            _same(got, want)
            if radius == 16:                                                      # equal peaks of the largest covariance a patch of bytes has: ambiguous exactly below ratio 1
                V = PP.VAR_MAX
                assert got[1][0].tolist() == [V, V, V] and got[2][0].tolist() == [V, V] and got[0][0].tolist() == [0, 0] and got[3][0] == (0 if ratio == 1024 else 3)
                assert got[0][1].tolist() == [0, -1] and got[0][2].tolist() == [0, 0] and got[1][2].tolist() == [V, V, V]
    c.close()


def test_device_form_with_and_without_each_output(ctxs):
    import torch
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A, 0, 1, 3, 13, n_rand=24); n = len(xyl)
    want = c.orb_patch_search(0, xyl, ref, 3, excl=1, min_var=4096, min_zncc_q10=920, peak_ratio_q10=RATIO)
    t_xyl = torch.from_numpy(xyl.copy()).cuda(); t_ref = torch.from_numpy(ref.copy()).cuda()
    shapes = ((n, 2), (n, 3), (n, 2), (n,), (5,))
    for mask in [1 << i for i in range(5)] + [31 ^ (1 << i) for i in range(5)] + [31]:
        outs = [torch.full(s, -77, dtype=torch.int32, device="cuda") for s in shapes]
        torch.cuda.synchronize()
        c.orb_patch_search_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), 3, 1, 1, 4096, 920, RATIO, *[o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)])
        c.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), want[i]) if mask >> i & 1 else bool((o == -77).all()), (mask, i)
    stats = torch.full((5,), -77, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    c.orb_patch_search_device(0, t_xyl.data_ptr(), 0, t_ref.data_ptr(), 3, stats_ptr=stats.data_ptr())      # n == 0: the counters are zeroed on the stream
    c.synchronize()
    assert stats.cpu().numpy().tolist() == [0] * 5


def test_every_refusal_leaves_the_context_usable(ctxs, vido):
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A, 0, 1, 3, 17, n_rand=24); xyl, ref = np.ascontiguousarray(xyl[:64]), np.ascontiguousarray(ref[:64])
    good = c.orb_patch_search(0, xyl, ref, 3)
    lib = c.lib; f = lib.vido_orb_patch_search
    dxy = np.empty((64, 2), np.int32); sums = np.empty((64, 3), np.int32); sec = np.empty((64, 2), np.int32); st = np.empty(64, np.int32); stats = np.full(5, -77, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(c.h).decode()
    out = (P(dxy), P(sums), P(sec), P(st), P(stats))
    call = lambda frame=0, x=P(xyl), n=64, blurred=1, r=P(ref), radius=3, excl=2, min_var=0, q=0, ratio=0, dev=0: f(c.h, frame, x, n, blurred, r, radius, excl, min_var, q, ratio, *out, dev)
    assert call(n=0) == 0 and stats.tolist() == [0] * 5                                                  # n == 0: successful no-op, stats zeroed
    assert f(c.h, 0, None, 0, 1, None, 3, 2, 0, 0, 0, None, None, None, None, None, 0) == 0
    for frame in (-1, 2, 1 << 20):                                                                       # the context was created for a batch of 2
        assert call(frame=frame) == -1 and "frame" in err()
    assert call(n=-1) == -1 and "point list" in err()
    assert call(x=None) == -1 and "point list" in err()
    assert call(r=None) == -1 and "reference" in err()
    for radius in (-1, 17, 1 << 20):
        assert call(radius=radius) == -1 and "radius" in err()
    for excl in (-1, 0, 17):
        assert call(excl=excl) == -1 and "excl" in err()
    assert call(min_var=-1) == -1 and "min_var" in err()
    for q in (-1, 1025):
        assert call(q=q) == -1 and "min_zncc_q10" in err()
        assert call(ratio=q) == -1 and "peak_ratio_q10" in err()
    assert call(x=C.c_void_p(P(xyl).value + 1), dev=1) == -1 and "aligned" in err()                      # device form, misaligned pointer: refused before any launch
    assert f(None, 0, P(xyl), 64, 1, P(ref), 3, 2, 0, 0, 0, *out, 0) == -1
    with pytest.raises(vido.VidoError):
        c.orb_patch_search(0, xyl, ref[:10], 3)
    if A["name"] == "64x64":                                                                             # a context without the blurred pyramid refuses blurred = 1, serves blurred = 0
        w, h, nl = SIZES["64x64"]
        c0 = vido.Context(width=w, height=h, max_batch=1, n_features=64, n_levels=nl, compute_descriptors=0)
        g = vido.synth.make_frame(w, h, seed=31); c0.orb_extract_batch(g[None], want_desc=False)
        assert c0.lib.vido_orb_patch_search(c0.h, 0, P(xyl), 64, 1, P(ref), 3, 2, 0, 0, 0, *out, 0) == -1 and "blurred pyramid" in c0.lib.vido_last_error(c0.h).decode()
        _same(c0.orb_patch_search(0, xyl, ref, 3, blurred=0, min_var=0, min_zncc_q10=512), R.patch_search([g], xyl, ref, 3, 2, 0, 512, 0))
        c0.close()
    _same(c.orb_patch_search(0, xyl, ref, 3), good)
