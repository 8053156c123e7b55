"""MI355X: vido_orb_patch_refine (csrc/patchrefine.hip k_patch_refine) against the numpy / Python-integer statement (tests/refimpl/patch_refine_np.py) on the level images
the context itself returns (vido_orb_read_level): q8, cost, iters, status and stats bit for bit, no tolerance anywhere.  Frames 64 x 64 (one level), 201 x 151 (odd size,
5 levels) and 1242 x 375 (8 levels); levels 0, 3 and the top one; both planes; max_shift_q8 0, 255, 256, 384, 512 (C = 0, 1, 1, 2, 2); iters 1, 6, 8; min_eig 0 and a
gating value; both sides of every border of rule 1; n across the wave and the four-point workgroup edge.

What every parametrised case must see (checked on the statement alone, before the kernel's outputs are looked at): the statuses -1, 0, 2 and 3, and status 0 at half of
the points at least.  Exempt, by the statement itself: at max_shift_q8 = 0 every step that is not (0, 0) leaves the window, so status 0 needs a reference that already sits
within 1/512 px and the half rule cannot hold there; with one iteration status 3 cannot occur at max_shift_q8 >= 256 (a step is clamped to +-256), which is why the statuses
are collected over the case's three iteration counts and not per count."""
import ctypes as C
import numpy as np
import pytest

from refimpl import patch_refine_np as R
from refimpl.patch_refine_np import constructed

pytestmark = pytest.mark.gpu

SIZES = {"64x64": (64, 64, 1), "201x151": (201, 151, 5), "1242x375": (1242, 375, 8)}
SHIFTS = (0, 255, 256, 384, 512)
COMBOS = ((1, 0), (6, 0), (8, 20000), (6, 20000))              # (iters, min_eig); 20 000 declines edge-like references (profiles/r19/patch_refine_cpu.txt: about half)
NAMES = ("q8", "cost", "iters", "status", "stats")


def _points(rng, lw, lh, level, n_levels, C_, n_rand):
    """x, y on both sides of every border of rule 1 (x - 3 - C >= 0, x + 3 + C <= w - 1) on all four sides, random interior points, random points around and beyond the
    level, huge coordinates and levels out of range."""
    xs = [2 + C_, 3 + C_, 4 + C_, lw - 5 - C_, lw - 4 - C_, lw - 3 - C_, lw // 2]; ys = [2 + C_, 3 + C_, lh - 4 - C_, lh - 3 - C_, lh // 2]
    pts = [(x, y, level) for x in xs for y in ys]
    r = np.stack([rng.randint(3 + C_, lw - 3 - C_, n_rand), rng.randint(3 + C_, lh - 3 - C_, n_rand), np.full(n_rand, level)], 1)
    o = np.stack([rng.randint(-8, lw + 8, n_rand // 6), rng.randint(-8, lh + 8, n_rand // 6), np.full(n_rand // 6, level)], 1)
    bad = [(20, 20, -1), (20, 20, n_levels), (20, 20, 1 << 20), (-(1 << 31), 20, level), ((1 << 31) - 1, 20, level), (20, -(1 << 31), level), (20, (1 << 31) - 1, level), (-1, -1, level)]
    return np.concatenate([np.array(pts), r, o, np.array(bad, np.int64)]).astype(np.int32)


def _references(rng, levels, xyl):
    """Per point, by k mod 6: (0, 1) the level resampled around the point at an offset drawn within +-1 px (1/256 px steps, denser towards 0 so that the 255 window holds most of them;
    the statement's own bilinear form; every third kind-0 point at offset 0: the level's own patch, status 0 at any window), (2) the same with noise, (3) the patch of another random place, (4) random bytes, (5) the constructed references in turn (flat, edge, ramp, checker ...)."""
    cons = [c["ref"] for c in constructed().values()]
    n = len(xyl); ref = np.empty((n, 64), np.uint8)
    for k, (x, y, l) in enumerate(xyl.astype(np.int64)):
        kind = k % 6
        lv = levels[l] if 0 <= l < len(levels) else levels[0]; h, w = lv.shape
        if kind in (0, 1, 2):
            sx, sy = int(min(max(x, 5), w - 6)), int(min(max(y, 5), h - 6))
            ox, oy = (0, 0) if k % 18 == 0 else tuple(int(v) for v in rng.randint(-256, 257, 2) * rng.randint(0, 257, 2) // 256)
            v = R.resample(lv, sx, sy, ox, oy).astype(np.float64)
        else:
            sx, sy = int(rng.randint(4, w - 3)), int(rng.randint(4, h - 3))
            v = lv[sy - 4:sy + 4, sx - 4:sx + 4].reshape(64).astype(np.float64)
        if kind == 2:
            v = v + rng.normal(0, 3, 64)
        elif kind == 4:
            v = rng.randint(0, 256, 64)
        elif kind == 5:
            v = cons[(k // 6) % len(cons)]
        ref[k] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return ref


def _inputs(levels, nl, shift, seed, n_rand=120):
    rng = np.random.RandomState(seed); C_ = (shift + 255) >> 8
    xyl = np.concatenate([_points(rng, levels[l].shape[1], levels[l].shape[0], l, nl, C_, n_rand) for l in sorted({0, min(3, nl - 1), nl - 1})])
    return xyl, _references(rng, levels, xyl)


def _statement_case(levels, nl, shift, seed):
    """inputs and the statement's outputs for the case's (iters, min_eig) combinations, with the two conditions every case must meet"""
    xyl, ref = _inputs(levels, nl, shift, seed)
    wants = [R.patch_refine(levels, xyl, ref, it, shift, me) for it, me in COMBOS]
    seen = set().union(*[set(w[3].tolist()) for w in wants])
    n0 = sum(int((w[3] == 0).sum()) for w in wants[:2]); n_all = 2 * len(xyl)            # the two runs without the gate
    for w in wants:
        assert w[4].sum() == len(xyl)
    assert seen == {-1, 0, 2, 3}, seen
    if shift > 0:
        assert 2 * n0 >= n_all, (n0, n_all)                                               # a kernel that declines everything cannot pass
    return xyl, ref, wants, (n0, n_all)


@pytest.fixture(scope="module", params=list(SIZES))
def ctxs(request, vido):
    """One context per frame size, batch of 2 with two different frames extracted; the level images of both planes read back once."""
    w, h, nl = SIZES[request.param]
    c = vido.Context(width=w, height=h, max_batch=2, n_features=500, n_levels=nl)
    c.orb_extract_batch(np.stack([vido.synth.make_frame(w, h, seed=31), vido.synth.make_canvas(h, w, seed=32, n_rect=30)]))
    planes = {(f, b): [c.orb_level(f, l, blurred=bool(b)) for l in range(nl)] for f in range(2) for b in range(2)}
    yield dict(c=c, nl=nl, planes=planes, name=request.param)
    c.close()


def _same(got, want):
    assert len(got) == len(want) == 5
    for g, w_, name in zip(got, want, NAMES):
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        if not np.array_equal(g, w_):
            bad = np.flatnonzero((g != w_).reshape(len(g), -1).any(1))
            assert False, (name, bad[:8], g[bad[:4]], w_[bad[:4]])


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("blurred", [0, 1])
def test_bit_equal_on_every_border_level_window_and_iteration_count(ctxs, blurred, shift):
    A = ctxs; c = A["c"]; levels = A["planes"][0, blurred]
    xyl, ref, wants, (n0, n_all) = _statement_case(levels, A["nl"], shift, 100 + shift)
    print("patch_refine %s blurred %d max_shift_q8 %d: %d points, statuses 0 2 3 -1 per (iters, min_eig) = %s, status 0 without the gate %d of %d" % (
        A["name"], blurred, shift, len(xyl), [w[4].tolist() for w in wants], n0, n_all))
    for (it, me), want in zip(COMBOS, wants):
        _same(c.orb_patch_refine(0, xyl, ref, it, shift, me, blurred=blurred), want)
    lw, lh = levels[0].shape[::-1]; st = wants[0][3]; C_ = (shift + 255) >> 8
    for x, y, ok in ((3 + C_, 3 + C_, True), (lw - 4 - C_, lh - 4 - C_, True), (2 + C_, 3 + C_, False), (3 + C_, 2 + C_, False), (lw - 3 - C_, 3 + C_, False), (3 + C_, lh - 3 - C_, False)):
        i = int(np.flatnonzero((xyl[:, 0] == x) & (xyl[:, 1] == y) & (xyl[:, 2] == 0))[0])
        assert bool(st[i] >= 0) == ok


def test_n_order_single_points_and_the_second_slab(ctxs):
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A["planes"][0, 1], A["nl"], 384, 5, n_rand=200)
    assert len(xyl) >= 257
    full = c.orb_patch_refine(0, xyl, ref, 6, 384, 0)
    _same(full, R.patch_refine(A["planes"][0, 1], xyl, ref, 6, 384, 0))
    cnt = lambda st: np.array([(st == s).sum() for s in (0, 2, 3, -1)], np.int32)
    for n in (0, 1, 3, 4, 5, 257):                                                # across the workgroup edge of four points; n == 0: empty outputs, stats zero
        got = c.orb_patch_refine(0, xyl[:n], ref[:n], 6, 384, 0)
        _same(got, tuple(v[:n] for v in full[:4]) + (cnt(full[3][:n]),))
    rev = c.orb_patch_refine(0, xyl[::-1], ref[::-1], 6, 384, 0)
    _same(tuple(v[::-1] for v in rev[:4]) + (rev[4],), full)
    for i in (0, 7, len(xyl) // 2, len(xyl) - 1):
        one = c.orb_patch_refine(0, xyl[i:i + 1], ref[i:i + 1], 6, 384, 0)
        _same(one, tuple(v[i:i + 1] for v in full[:4]) + (cnt(full[3][i:i + 1]),))
    for b in (0, 1):                                                              # slab 1 of the batch of 2: the other frame, references from it
        x1, r1 = _inputs(A["planes"][1, b], A["nl"], 256, 11, n_rand=24)
        got = c.orb_patch_refine(1, x1, r1, 6, 256, 0, blurred=b)
        _same(got, R.patch_refine(A["planes"][1, b], x1, r1, 6, 256, 0))
        assert not np.array_equal(got[1], c.orb_patch_refine(0, x1, r1, 6, 256, 0, blurred=b)[1])


def test_constructed_patches_uploaded_as_a_frame(vido):
    """The constructed tiles (flat, edge, ramp, the 2-px checker at the largest H, its inverse at the largest |e|, the shifted checker at the largest products, the bowl
    that leaves the window, the pair of known offset) pasted into a frame and refined on the unblurred level 0, where the level IS the uploaded image."""
    w, h, nl = SIZES["201x151"]
    cases = constructed(); names = sorted(cases); T = R.TILE
    img = vido.synth.make_frame(w, h, seed=9).copy()
    xyl = []; ref = []
    for i, name in enumerate(names):
        x0, y0 = 8 + 22 * (i % 8), 10 + 30 * (i // 8)
        img[y0:y0 + T, x0:x0 + T] = cases[name]["img"]; xyl.append((x0 + 8, y0 + 8, 0)); ref.append(cases[name]["ref"])
    xyl = np.array(xyl, np.int32); ref = np.stack(ref)
    c = vido.Context(width=w, height=h, max_batch=1, n_features=500, n_levels=nl)
    c.orb_extract(img)
    assert np.array_equal(c.orb_level(0, 0), img)
    for it, shift, me in ((6, 384, 0), (1, 512, 0), (8, 512, 0), (8, 0, 0), (6, 255, 1), (6, 384, 2 ** 31 - 1)):
        want = R.patch_refine([img], xyl, ref, it, shift, me)
        got = c.orb_patch_refine(0, xyl, ref, it, shift, me, blurred=0)
        _same(got, want)
        if (it, shift, me) == (6, 384, 0):
            for i, name in enumerate(names):
                cs = cases[name]
                assert cs["status"] is None or got[3][i] == cs["status"], name
                if name == "known_offset":
                    assert np.abs(got[0][i] - np.array(cs["q8"])).max() <= 1
                if name == "checker_inverse":
                    assert got[1][i, 0] == 36 * 36 * 65280 * 65280                 # |e| = 65 280 on all 36 pixels, half of each sign: cost = n sum e^2
    c.close()


def test_device_form_with_and_without_each_output(ctxs):
    import torch
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A["planes"][0, 1], A["nl"], 384, 13, n_rand=24); n = len(xyl)
    want = c.orb_patch_refine(0, xyl, ref, 6, 384, 0)
    t_xyl = torch.from_numpy(xyl.copy()).cuda(); t_ref = torch.from_numpy(ref.copy()).cuda()
    shapes = ((n, 2), (n, 2), (n,), (n,), (4,)); dtypes = (torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)
    for mask in [1 << i for i in range(5)] + [31 ^ (1 << i) for i in range(5)] + [31]:
        outs = [torch.full(s, -77, dtype=d, device="cuda") for s, d in zip(shapes, dtypes)]
        torch.cuda.synchronize()
        c.orb_patch_refine_device(0, t_xyl.data_ptr(), n, t_ref.data_ptr(), 6, 384, 0, 1, *[o.data_ptr() if mask >> i & 1 else None for i, o in enumerate(outs)])
        c.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), want[i]) if mask >> i & 1 else bool((o == -77).all()), (mask, i)
    stats = torch.full((4,), -77, dtype=torch.int32, device="cuda"); torch.cuda.synchronize()
    c.orb_patch_refine_device(0, t_xyl.data_ptr(), 0, t_ref.data_ptr(), stats_ptr=stats.data_ptr())      # n == 0: the counters are zeroed on the stream
    c.synchronize()
    assert stats.cpu().numpy().tolist() == [0] * 4


def test_every_refusal_leaves_the_context_usable(ctxs, vido):
    A = ctxs; c = A["c"]
    xyl, ref = _inputs(A["planes"][0, 1], A["nl"], 384, 17, n_rand=24); xyl, ref = np.ascontiguousarray(xyl[:64]), np.ascontiguousarray(ref[:64])
    good = c.orb_patch_refine(0, xyl, ref, 6, 384, 0)
    lib = c.lib; f = lib.vido_orb_patch_refine
    q8 = np.empty((64, 2), np.int32); cost = np.empty((64, 2), np.int64); it = np.empty(64, np.int32); st = np.empty(64, np.int32); stats = np.full(4, -77, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vido_last_error(c.h).decode()
    out = (P(q8), P(cost), P(it), P(st), P(stats))
    call = lambda frame=0, x=P(xyl), n=64, blurred=1, r=P(ref), iters=6, shift=384, eig=0, dev=0, o=out: f(c.h, frame, x, n, blurred, r, iters, shift, eig, *o, dev)
    assert call(n=0) == 0 and stats.tolist() == [0] * 4                                                  # n == 0: successful no-op, stats zeroed
    assert f(c.h, 0, None, 0, 1, None, 6, 384, 0, None, None, None, None, None, 0) == 0
    for frame in (-1, 2, 1 << 20):                                                                       # the context was created for a batch of 2
        assert call(frame=frame) == -1 and "frame" in err()
    assert call(n=-1) == -1 and "point list" in err()
    assert call(x=None) == -1 and "point list" in err()
    assert call(r=None) == -1 and "reference" in err()
    for iters in (-1, 0, 9, 1 << 20):
        assert call(iters=iters) == -1 and "iters" in err()
    for shift in (-1, 513, 1 << 20):
        assert call(shift=shift) == -1 and "max_shift_q8" in err()
    assert call(eig=-1) == -1 and "min_eig" in err()
    assert call(x=C.c_void_p(P(xyl).value + 1), dev=1) == -1 and "aligned" in err()                      # device form, misaligned pointer: refused before any launch
    assert call(dev=1, o=(P(q8), C.c_void_p(P(cost).value + 4), P(it), P(st), P(stats))) == -1 and "aligned" in err()      # cost_out is 8-byte data
    assert f(None, 0, P(xyl), 64, 1, P(ref), 6, 384, 0, *out, 0) == -1
    with pytest.raises(vido.VidoError):
        c.orb_patch_refine(0, xyl, ref[:10])
    if A["name"] == "64x64":                                                                             # a context without the blurred pyramid refuses blurred = 1, serves blurred = 0
        w, h, nl = SIZES["64x64"]
        c0 = vido.Context(width=w, height=h, max_batch=1, n_features=64, n_levels=nl, compute_descriptors=0)
        g = vido.synth.make_frame(w, h, seed=31); c0.orb_extract_batch(g[None], want_desc=False)
        assert c0.lib.vido_orb_patch_refine(c0.h, 0, P(xyl), 64, 1, P(ref), 6, 384, 0, *out, 0) == -1 and "blurred pyramid" in c0.lib.vido_last_error(c0.h).decode()
        _same(c0.orb_patch_refine(0, xyl, ref, 6, 384, 0, blurred=0), R.patch_refine([g], xyl, ref, 6, 384, 0))
        c0.close()
    _same(c.orb_patch_refine(0, xyl, ref, 6, 384, 0), good)
