"""MI355X: vido_orb_patch_points (csrc/patchpts.hip k_patch_points) against the numpy / Python-integer statement (tests/refimpl/patch_points_np.py) on the level images
the context itself returns (vido_orb_read_level): patch_out, sums_out and status_out bit for bit, no tolerance anywhere.  Shapes: 64 x 64 (one level), 201 x 151 (odd
size, pitch 256, 5 levels) and 1242 x 375 (8 levels); level 0 and the top level; both planes; every border; n across the four-point workgroup edge."""
import ctypes as C
import numpy as np
import pytest

from refimpl import patch_points_np as R
from refimpl.patch_points_np import constructed

pytestmark = pytest.mark.gpu

SIZES = {"64x64": (64, 64, 1), "201x151": (201, 151, 5), "1242x375": (1242, 375, 8)}
THRESHOLDS = (0, 1, 512, 1024)


def _points(rng, lw, lh, level, n_levels, n_rand):
    """Every combination of x, y in {3, 4, w-5, w-4, w-3} (on the border of validity, just inside and just outside it), random interior points (x = 0 .. 3 mod 4 all occur),
    points around and beyond the image, negative and huge coordinates, and levels out of range."""
    xs = [3, 4, 5, 6, 7, lw - 5, lw - 4, lw - 3, lw // 2]; ys = [3, 4, lh - 5, lh - 4, lh - 3, lh // 2]
    pts = [(x, y, level) for x in xs for y in ys]
    r = np.stack([rng.randint(4, lw - 3, n_rand), rng.randint(4, lh - 3, n_rand), np.full(n_rand, level)], 1)
    o = np.stack([rng.randint(-6, lw + 6, n_rand // 4), rng.randint(-6, lh + 6, n_rand // 4), np.full(n_rand // 4, level)], 1)
    bad = [(20, 20, -1), (20, 20, n_levels), (20, 20, 1 << 20), (-(1 << 31), 20, level), ((1 << 31) - 1, 20, level), (20, -(1 << 31), level), (20, (1 << 31) - 1, level), (-1, -1, level)]
    return np.concatenate([np.array(pts), r, o, np.array(bad, np.int64)]).astype(np.int32)


def _references(rng, own):
    """Reference patches per point: the point's own patch (the equality case: cov^2 == var var), the own patch with noise of three strengths (verdicts on both sides of
    every threshold), a gain / offset copy, its inverse, random bytes, a constant."""
    n = len(own); ref = np.empty((n, 64), np.uint8)
    for k in range(n):
        o = own[k].astype(np.float64); kind = k % 8
        if kind == 0:
            v = o
        elif kind in (1, 2, 3):
            v = o + rng.normal(0, (3, 12, 40)[kind - 1], 64)
        elif kind == 4:
            v = 0.5 * o + 40
        elif kind == 5:
            v = 255 - o
        elif kind == 6:
            v = rng.randint(0, 256, 64)
        else:
            v = np.full(64, 99.0)
        ref[k] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return ref


@pytest.fixture(scope="module", params=list(SIZES))
def ctxs(request, vido):
    """One context per frame size, batch of 2 with two different frames extracted; the level images of both planes read back once; points and references for level 0 and
    the top level, drawn once."""
    w, h, nl = SIZES[request.param]
    c = vido.Context(width=w, height=h, max_batch=2, n_features=500, n_levels=nl)
    c.orb_extract_batch(np.stack([vido.synth.make_frame(w, h, seed=31), vido.synth.make_canvas(h, w, seed=32, n_rect=30)]))
    planes = {(f, b): [c.orb_level(f, l, blurred=bool(b)) for l in range(nl)] for f in range(2) for b in range(2)}
    rng = np.random.RandomState(9)
    xyl = np.concatenate([_points(rng, planes[0, 0][l].shape[1], planes[0, 0][l].shape[0], l, nl, 600) for l in sorted({0, nl - 1})])
    own = R.take(planes[0, 1], xyl)[0]
    yield dict(c=c, nl=nl, planes=planes, xyl=xyl, ref=_references(rng, own), name=request.param)
    c.close()


def _same(got, want):
    for g, w_ in zip(got, want):
        assert (g is None) == (w_ is None)
        if g is not None:
            assert g.dtype == w_.dtype and np.array_equal(g, w_)


@pytest.mark.parametrize("blurred", [0, 1])
def test_bit_equal_on_every_border_level_and_threshold(ctxs, blurred):
    A = ctxs; c, xyl, ref = A["c"], A["xyl"], A["ref"]
    levels = A["planes"][0, blurred]
    seen = set()
    for q in THRESHOLDS:
        for min_var in (0, 1, 147456):
            want = R.patch_points(levels, xyl, ref, min_var, q)
            _same(c.orb_patch_points(0, xyl, ref, blurred=blurred, min_var=min_var, min_zncc_q10=q), want)
            seen |= set(want[2].tolist())
    assert seen == {-1, 0, 1, 2}
    valid = want[2] >= 0
    assert valid.sum() > 1000 // (1 if A["nl"] > 1 else 2) and (~valid).sum() > 60
    assert {int(v) for v in xyl[valid, 0] & 3} == {0, 1, 2, 3}                   # every alignment of a row start
    lw, lh = levels[0].shape[::-1]
    for x, y, ok in ((4, 4, True), (lw - 4, lh - 4, True), (3, 4, False), (4, 3, False), (lw - 3, 4, False), (4, lh - 3, False)):
        i = int(np.flatnonzero((xyl[:, 0] == x) & (xyl[:, 1] == y) & (xyl[:, 2] == 0))[0])
        assert bool(valid[i]) == ok
    _same(c.orb_patch_points(0, xyl, blurred=blurred), (want[0], None, None))     # the "take the patches" form
    if blurred:                                                                   # own patch as the reference: accepted at 1024 whenever it has any texture at all
        st = c.orb_patch_points(0, xyl[::8], ref[::8], blurred=1, min_var=1, min_zncc_q10=1024)
        assert np.array_equal(st[1][:, 0], st[1][:, 1]) and np.array_equal(st[1][:, 1], st[1][:, 2]) and set(st[2].tolist()) <= {-1, 0, 2} and (st[2] == 0).sum() > 50


def test_n_order_single_points_and_the_second_slab(ctxs):
    A = ctxs; c, xyl, ref = A["c"], A["xyl"], A["ref"]
    full = c.orb_patch_points(0, xyl, ref, min_var=4096, min_zncc_q10=920)
    _same(full, R.patch_points(A["planes"][0, 1], xyl, ref, 4096, 920))
    for n in (0, 1, 3, 4, 5, 257):                                                # across the workgroup edge of four points
        got = c.orb_patch_points(0, xyl[:n], ref[:n], min_var=4096, min_zncc_q10=920)
        _same(got, tuple(v[:n] for v in full))
    rev = c.orb_patch_points(0, xyl[::-1], ref[::-1], min_var=4096, min_zncc_q10=920)
    _same(tuple(v[::-1] for v in rev), full)
    for i in (0, 7, len(xyl) // 2, len(xyl) - 1):
        one = c.orb_patch_points(0, xyl[i:i + 1], ref[i:i + 1], min_var=4096, min_zncc_q10=920)
        _same(one, tuple(v[i:i + 1] for v in full))
    for b in (0, 1):                                                              # slab 1 of the batch of 2: the other frame
        got = c.orb_patch_points(1, xyl, ref, blurred=b, min_var=4096, min_zncc_q10=512)
        _same(got, R.patch_points(A["planes"][1, b], xyl, ref, 4096, 512))
    assert not np.array_equal(got[0], full[0])


def test_constructed_patches_uploaded_as_a_frame(vido):
    """The CPU test's constructed pairs: the current patches are pasted into a 201 x 151 frame at x = 0 .. 3 mod 4 and read from the unblurred level 0, where the patch IS
    the uploaded image; sums and verdicts are the closed forms."""
    w, h, nl = SIZES["201x151"]
    cases = constructed(); names = sorted(cases)
    img = np.full((h, w), 128, np.uint8); xyl = []
    for i, name in enumerate(names):
        x, y = 8 + 21 * i + (i & 3), 12 + 9 * (i % 5)
        img[y - 4:y + 4, x - 4:x + 4] = cases[name][1].reshape(8, 8); xyl.append((x, y, 0))
    xyl = np.array(xyl, np.int32); ref = np.stack([cases[nm][0] for nm in names])
    c = vido.Context(width=w, height=h, max_batch=1, n_features=500, n_levels=nl)
    c.orb_extract(img)
    assert np.array_equal(c.orb_level(0, 0), img)
    for q in THRESHOLDS:
        for min_var in (0, 1):
            patch, sums, st = c.orb_patch_points(0, xyl, ref, blurred=0, min_var=min_var, min_zncc_q10=q)
            assert np.array_equal(patch, np.stack([cases[nm][1] for nm in names]))
            _same((patch, sums, st), R.patch_points([img], xyl, ref, min_var, q))
            S = dict(zip(names, zip(sums.tolist(), st.tolist())))
            assert S["identical"][1] == 0 and S["checker"] == ([66585600] * 3, 0) and S["gain_offset"][1] == 0          # equality cases, accepted even at 1024
            assert S["inverse"][1] == 1 and S["checker_inverse"] == ([-66585600, 66585600, 66585600], 1)                # cov < 0: rejected even at 0
            assert S["white"] == ([0, 0, 0], 2 if min_var else 1)
            assert S["flat_vs_random"][1] == (2 if min_var else 1)
    c.close()


def test_device_form_with_and_without_each_output(ctxs):
    import torch
    A = ctxs; c, xyl, ref = A["c"], A["xyl"], A["ref"]
    n = len(xyl)
    want = c.orb_patch_points(0, xyl, ref, min_var=4096, min_zncc_q10=920)
    t_xyl = torch.from_numpy(xyl.copy()).cuda(); t_ref = torch.from_numpy(ref.copy()).cuda()
    for mask in range(1, 8):
        t_patch = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda"); t_sums = torch.full((n, 3), -77, dtype=torch.int32, device="cuda"); t_st = torch.full((n,), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.orb_patch_points_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), 1, 4096, 920, t_patch.data_ptr() if mask & 1 else None, t_sums.data_ptr() if mask & 2 else None,
                                  t_st.data_ptr() if mask & 4 else None)
        c.synchronize()
        assert np.array_equal(t_patch.cpu().numpy(), want[0]) if mask & 1 else bool((t_patch == 0xA5).all())
        assert np.array_equal(t_sums.cpu().numpy(), want[1]) if mask & 2 else bool((t_sums == -77).all())
        assert np.array_equal(t_st.cpu().numpy(), want[2]) if mask & 4 else bool((t_st == -77).all())
    t_patch = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    c.orb_patch_points_device(0, t_xyl.data_ptr(), n, None, 0, 0, 0, t_patch.data_ptr())                 # no reference: the patches of the unblurred plane
    c.synchronize()
    assert np.array_equal(t_patch.cpu().numpy(), R.take(A["planes"][0, 0], xyl)[0])


def test_every_refusal_leaves_the_context_usable(ctxs, vido):
    A = ctxs; c = A["c"]; xyl, ref = np.ascontiguousarray(A["xyl"][:64]), np.ascontiguousarray(A["ref"][:64])
    good = c.orb_patch_points(0, xyl, ref)
    lib = c.lib; f = lib.vido_orb_patch_points
    patch = np.empty((64, 64), np.uint8); sums = np.empty((64, 3), np.int32); st = np.empty(64, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(c.h).decode()
    assert f(c.h, 0, P(xyl), 0, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 0) == 0                       # n == 0: successful no-op
    assert f(c.h, 0, None, 0, 1, None, 0, 0, None, None, None, 0) == 0
    for frame in (-1, 2, 1 << 20):                                                                       # the context was created for a batch of 2
        assert f(c.h, frame, P(xyl), 64, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 0) == -1 and "frame" in err()
    assert f(c.h, 0, P(xyl), -1, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 0) == -1 and "point list" in err()
    assert f(c.h, 0, None, 64, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 0) == -1 and "point list" in err()
    assert f(c.h, 0, P(xyl), 64, 1, None, 0, 0, P(patch), P(sums), None, 0) == -1 and "reference" in err()            # sums without reference patches
    assert f(c.h, 0, P(xyl), 64, 1, None, 0, 0, P(patch), None, P(st), 0) == -1 and "reference" in err()              # verdicts without reference patches
    assert f(c.h, 0, P(xyl), 64, 1, P(ref), -1, 0, P(patch), P(sums), P(st), 0) == -1 and "min_var" in err()
    for q in (-1, 1025):
        assert f(c.h, 0, P(xyl), 64, 1, P(ref), 0, q, P(patch), P(sums), P(st), 0) == -1 and "min_zncc_q10" in err()
    assert f(c.h, 0, C.c_void_p(P(xyl).value + 1), 64, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 1) == -1 and "aligned" in err()      # device form, misaligned pointer: refused before any launch
    assert f(None, 0, P(xyl), 64, 1, P(ref), 0, 0, P(patch), P(sums), P(st), 0) == -1
    with pytest.raises(vido.VidoError):
        c.orb_patch_points(0, xyl, ref[:10])
    if A["name"] == "64x64":                                                                             # a context without the blurred pyramid refuses blurred = 1, serves blurred = 0
        w, h, nl = SIZES["64x64"]
        c0 = vido.Context(width=w, height=h, max_batch=1, n_features=64, n_levels=nl, compute_descriptors=0)
        g = vido.synth.make_frame(w, h, seed=31); c0.orb_extract_batch(g[None], want_desc=False)
        assert c0.lib.vido_orb_patch_points(c0.h, 0, P(xyl), 64, 1, None, 0, 0, P(patch), None, None, 0) == -1 and "blurred pyramid" in c0.lib.vido_last_error(c0.h).decode()
        _same(c0.orb_patch_points(0, xyl, ref, blurred=0, min_var=0, min_zncc_q10=512), R.patch_points([g], xyl, ref, 0, 512))
        c0.close()
    _same(c.orb_patch_points(0, xyl, ref), good)
