"""CPU: the numpy / Python-integer statement of vido_orb_patch_search (tests/refimpl/patch_search_np.py) against a brute-force float64 ZNCC and on constructed images whose
answer follows from the definition alone.  No GPU; tests/test_patch_search_gpu.py holds the kernel to this statement bit for bit."""
import numpy as np
import pytest

from refimpl import patch_points_np as PP
from refimpl import patch_search_np as R
from refimpl.patch_points_np import constructed


def _zncc64(a, b):
    a = a.astype(np.float64).ravel(); b = b.astype(np.float64).ravel()
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return None if den == 0 else float((da * db).sum() / den)


def _brute(img, x, y, a, radius):
    """{(dx, dy): float64 ZNCC} over the candidates whose patch lies wholly inside img and has any variance at all"""
    h, w = img.shape; out = {}
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            px, py = x + dx, y + dy
            if px < 4 or px + 3 >= w or py < 4 or py + 3 >= h:
                continue
            z = _zncc64(a, img[py - 4:py + 4, px - 4:px + 4])
            if z is not None:
                out[dx, dy] = z
    return out


def _noise(seed, h=64, w=72):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def _plant(img, x, y, patch):
    img[y - 4:y + 4, x - 4:x + 4] = patch.reshape(8, 8)


def test_a_planted_patch_is_found_where_it_was_planted():
    rng = np.random.RandomState(1)
    for radius in (1, 3, 8, 16):
        for _ in range(6):
            img = _noise(rng.randint(1 << 30)); a = rng.randint(0, 256, 64).astype(np.uint8)
            dx, dy = (int(v) for v in rng.randint(-radius, radius + 1, 2))
            _plant(img, 36 + dx, 32 + dy, a)
            st, dxy, sm, sec = R.search_one([img], 36, 32, 0, a, radius, 2, 147456, 920, 0)
            assert st == 0 and dxy == (dx, dy) and sm[0] == sm[1] == sm[2] == PP.sums(a, a)[1]
            z = _brute(img, 36, 32, a, radius)
            assert max(z, key=z.get) == (dx, dy) and abs(z[dx, dy] - 1.0) < 1e-12
            if sec != (0, 0):                                                  # the runner-up is the float64 runner-up outside the peak's own neighbourhood
                zo = {k: v for k, v in z.items() if max(abs(k[0] - dx), abs(k[1] - dy)) > 2 and v > 0}
                srt = sorted(zo.values())
                if len(srt) > 1 and srt[-1] - srt[-2] > 1e-9:
                    assert abs(sec[0] / np.sqrt(float(sm[1]) * sec[1]) - srt[-1]) < 1e-12


def test_order_agrees_with_float64_on_textured_images():
    """smooth random images (a ZNCC peak several pixels wide): the integer order picks the float64 maximum wherever that maximum is clear of the next value by 1e-9, and the
    gate is the float gate wherever the value is clear of the threshold."""
    rng = np.random.RandomState(2); n_dec = 0; seen = set()
    for i in range(40):
        base = rng.uniform(0, 255, (20, 22)); img = np.kron(base, np.ones((4, 4)))[:64, :72]
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        x, y = int(rng.randint(4, 68)), int(rng.randint(4, 60)); radius = (3, 8)[i % 2]
        ox, oy = (int(v) for v in rng.randint(-radius, radius + 1, 2))
        sx, sy = min(max(x + ox, 4), 68), min(max(y + oy, 4), 60)
        a = np.clip(img[sy - 4:sy + 4, sx - 4:sx + 4].astype(np.float64) * 0.8 + 20 + rng.normal(0, (2, 10, 40)[i % 3], (8, 8)), 0, 255).astype(np.uint8).reshape(64)
        for min_var, q in ((0, 0), (147456, 920), (4096, 512)):
            st, dxy, sm, sec = R.search_one([img], x, y, 0, a, radius, 2, min_var, q, 0)
            seen.add(st)
            z = {k: v for k, v in _brute(img, x, y, a, radius).items() if v > 0 and PP.sums(a, img[y + k[1] - 4:y + k[1] + 4, x + k[0] - 4:x + k[0] + 4])[2] >= min_var}
            if PP.sums(a, a)[1] < min_var:
                assert st == 2
                continue
            if not z:
                assert st == 1 and dxy == (0, 0)
                continue
            srt = sorted(z.items(), key=lambda kv: -kv[1])
            if len(srt) > 1 and srt[0][1] - srt[1][1] <= 1e-9:
                continue
            assert dxy == srt[0][0]
            if abs(srt[0][1] - q / 1024.0) > 1e-9:
                n_dec += 1
                assert st == (0 if srt[0][1] >= q / 1024.0 else 1)
    assert n_dec > 60 and {0, 1} <= seen


def test_two_equal_plants_nearer_then_smaller_dy_then_smaller_dx():
    a = np.random.RandomState(3).randint(0, 256, 64).astype(np.uint8); v = PP.sums(a, a)[1]
    for (p, q), want in ((((5, 0), (-10, 0)), (5, 0)), (((0, 10), (10, 0)), (10, 0)), (((-10, 0), (10, 0)), (-10, 0)), (((0, -10), (-10, 0)), (0, -10)), (((6, 8), (10, 0)), (10, 0)),
                         (((-6, -8), (10, 0)), (-6, -8))):
        img = _noise(4)
        _plant(img, 36 + p[0], 32 + p[1], a); _plant(img, 36 + q[0], 32 + q[1], a)
        st, dxy, sm, sec = R.search_one([img], 36, 32, 0, a, 12, 2, 147456, 920, 0)
        assert (st, dxy, sm, sec) == (0, want, (v, v, v), (v, v))                    # the other plant is the runner-up: as good, outside the peak
        assert R.search_one([img], 36, 32, 0, a, 12, 2, 147456, 920, 1000)[0] == 3   # ... which the peak test calls ambiguous
        assert R.search_one([img], 36, 32, 0, a, 12, 2, 147456, 920, 1024)[0] == 0   # ZNCC2 > 1.0 ZNCC1 is false on equality
        assert R.search_one([img], 36, 32, 0, a, 8, 16, 147456, 0, 1000)[3] == (0, 0)     # excl covers the whole window: no second, whatever the best is


def test_periodic_texture_is_ambiguous_only_with_the_peak_test_on():
    rng = np.random.RandomState(5)
    tile = rng.randint(0, 256, (64, 5)).astype(np.uint8); img = np.tile(tile, (1, 15))[:, :72]      # period 5 in x > excl = 2
    a = img[28:36, 32:40].reshape(64).copy(); v = PP.sums(a, a)[1]
    st, dxy, sm, sec = R.search_one([img], 36, 32, 0, a, 8, 2, 147456, 920, 0)
    assert (st, dxy, sm, sec) == (0, (0, 0), (v, v, v), (v, v))                       # equal peaks at dx = 0, +-5: the nearest wins, the runner-up is as good
    assert R.search_one([img], 36, 32, 0, a, 8, 2, 147456, 920, 922)[0] == 3
    assert R.search_one([img], 36, 32, 0, a, 8, 5, 147456, 920, 922)[0] == 0         # excl swallows the neighbouring periods: within radius 8 only dx = 0, +-5 repeat
    assert R.search_one([img], 36, 32, 0, a, 4, 2, 147456, 920, 922)[0] == 0         # radius below the period: one peak


def test_checkerboards_at_var_max_do_not_wrap():
    C = constructed(); chk = C["checker"][0]; inv = C["checker_inverse"][1]
    yy, xx = np.mgrid[0:64, 0:72]; img = (((yy + xx) & 1) * 255).astype(np.uint8)
    for a, first in ((chk, (0, 0)), (inv, (0, -1))):                                  # the inverse matches at odd offsets: d2 = 1, smallest dy
        st, dxy, sm, sec = R.search_one([img], 36, 32, 0, a, 16, 1, 147456, 1024, 0)
        assert (st, dxy, sm) == (0, first, (R_VAR, R_VAR, R_VAR)) and sec == (R_VAR, R_VAR)
        assert R_VAR ** 3 * 1024 * 1024 > 2 ** 96                                     # the peak test's sides really are near 2^98
        assert R.search_one([img], 36, 32, 0, a, 16, 1, 147456, 1024, 1024)[0] == 0 and R.search_one([img], 36, 32, 0, a, 16, 1, 147456, 1024, 1023)[0] == 3
        assert R.search_one([img], 36, 32, 0, a, 0, 1, 147456, 1024, 0)[0] == (0 if first == (0, 0) else 1)      # radius 0 on the inverse: cov < 0, no eligible candidate
    assert R.before((R_VAR, R_VAR, 1, 0), (R_VAR - 1, R_VAR, 0, 0)) and not R.before((R_VAR - 1, R_VAR, 0, 0), (R_VAR, R_VAR, 1, 0))


R_VAR = PP.VAR_MAX


def test_flat_reference_window_partly_and_wholly_outside():
    img = _noise(6); a = np.random.RandomState(7).randint(0, 256, 64).astype(np.uint8)
    assert R.search_one([img], 36, 32, 0, np.full(64, 17, np.uint8), 8, 2, 1, 0, 0) == (2, (0, 0), (0, 0, 0), (0, 0))
    lowc = (100 + np.arange(64) % 3).astype(np.uint8); vl = PP.sums(lowc, lowc)[1]
    assert R.search_one([img], 36, 32, 0, lowc, 8, 2, vl + 1, 0, 0) == (2, (0, 0), (0, vl, 0), (0, 0)) and R.search_one([img], 36, 32, 0, lowc, 8, 2, vl, 0, 0)[0] != 2
    assert R.search_one([img], -100, -100, 0, np.full(64, 17, np.uint8), 8, 2, 1, 0, 0)[0] == -1                  # invalid comes before no texture
    # partly outside: the point itself has no patch (x = 1), candidates from dx = 3 on do; the plant at x = 6 is found
    _plant(img, 6, 5, a)
    st, dxy, sm, sec = R.search_one([img], 1, 2, 0, a, 8, 2, 147456, 920, 0)
    assert (st, dxy) == (0, (5, 3)) and set(_brute(img, 1, 2, a, 8)) == {(dx, dy) for dx in range(3, 9) for dy in range(2, 9)}
    st, dxy, sm, sec = R.search_one([img], 75, 63, 0, a, 8, 2, 0, 0, 0)                                       # bottom right: candidates x <= 68, y <= 60 only
    assert st in (0, 1) and dxy[0] <= -7 and dxy[1] <= -3
    for x, y, l in ((-5, 32, 0), (36, -5, 0), (77, 32, 0), (36, 69, 0), (36, 32, 1), (36, 32, -1), (1 << 31, 32, 0), (-(1 << 31), 32, 0)):
        assert R.search_one([img], x, y, l, a, 8, 2, 0, 0, 0) == (-1, (0, 0), (0, 0, 0), (0, 0))
    assert R.search_one([img], -4, 32, 0, a, 8, 2, 0, 0, 0)[0] != -1 and R.search_one([img], 76, 32, 0, a, 8, 2, 0, 0, 0)[0] != -1      # x + 8 = 4 and x - 8 = w - 4: one column
    for bad in ((17, 2, 0, 0, 0), (-1, 2, 0, 0, 0), (8, 0, 0, 0, 0), (8, 17, 0, 0, 0), (8, 2, -1, 0, 0), (8, 2, 0, 1025, 0), (8, 2, 0, 0, 1025), (8, 2, 0, 0, -1)):
        with pytest.raises(ValueError):
            R.search_one([img], 36, 32, 0, a, *bad)


def test_radius_zero_is_patch_points_but_for_a_textureless_current_patch():
    rng = np.random.RandomState(8)
    img = _noise(9); img[20:40, 20:50] = 90                                          # a flat area: current patches without texture
    xyl = np.stack([rng.randint(-2, 76, 400), rng.randint(-2, 68, 400), rng.randint(-1, 2, 400)], 1)
    own = PP.take([img], xyl)[0]
    ref = np.where(rng.uniform(size=(400, 1)) < 0.5, np.clip(own + rng.normal(0, 12, own.shape), 0, 255), rng.randint(0, 256, own.shape)).astype(np.uint8)
    ref[::9] = 50
    n_diff = 0
    for min_var, q in ((0, 0), (4096, 512), (147456, 920), (147456, 1024)):
        _, psm, pst = PP.patch_points([img], xyl, ref, min_var, q)
        dxy, sm, sec, st, stats = R.patch_search([img], xyl, ref, 0, 1, min_var, q, 1000)
        assert not dxy.any() and not sec.any() and stats.sum() == 400 and [int((st == s).sum()) for s in (0, 1, 2, 3, -1)] == stats.tolist()
        for k in range(400):
            if pst[k] == 2 and psm[k, 1] >= min_var:                                 # the stated difference: textured reference, textureless current patch
                assert st[k] == 1 and tuple(sm[k]) == (0, psm[k, 1], 0); n_diff += 1
            elif pst[k] == 1 and psm[k, 0] <= 0:                                     # cov <= 0: not eligible, so the sums are those of "no best"
                assert st[k] == 1 and tuple(sm[k]) == (0, psm[k, 1], 0)
            elif pst[k] == 2:
                assert st[k] == 2 and tuple(sm[k]) == (0, psm[k, 1], 0)
            else:
                assert st[k] == pst[k] and np.array_equal(sm[k], psm[k])
    assert n_diff > 10


def _slow(levels, x, y, level, a, radius, excl, min_var, q, ratio):
    """the statement once more, literally: patch_points_np.take and .sums per candidate, Python integers throughout"""
    if not 0 <= level < len(levels):
        return -1, (0, 0), (0, 0, 0), (0, 0)
    offs = [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    patch, valid = PP.take(levels, [(x + dx, y + dy, level) for dx, dy in offs])
    if not valid.any():
        return -1, (0, 0), (0, 0, 0), (0, 0)
    var_ref = PP.sums(a, a)[1]
    if var_ref < min_var:
        return 2, (0, 0), (0, var_ref, 0), (0, 0)
    elig = []
    for (dx, dy), b, ok in zip(offs, patch, valid):
        if ok:
            cov, _, vc = PP.sums(a, b)
            if vc >= min_var and cov > 0:
                elig.append((cov, vc, dx, dy))
    def first(cs):
        best = None
        for c in cs:
            if best is None or c[0] * c[0] * best[1] > best[0] * best[0] * c[1] or (c[0] * c[0] * best[1] == best[0] * best[0] * c[1] and
                                                                                      (c[2] ** 2 + c[3] ** 2, c[3], c[2]) < (best[2] ** 2 + best[3] ** 2, best[3], best[2])):
                best = c
        return best
    b1 = first(elig)
    if b1 is None:
        return 1, (0, 0), (0, var_ref, 0), (0, 0)
    b2 = first([c for c in elig if max(abs(c[2] - b1[2]), abs(c[3] - b1[3])) > excl])
    sec = (b2[0], b2[1]) if b2 else (0, 0)
    if b1[0] ** 2 * 1024 ** 2 < q * q * var_ref * b1[1]:
        st = 1
    elif ratio and b2 and b2[0] ** 2 * b1[1] * 1024 ** 2 > ratio * ratio * b1[0] ** 2 * b2[1]:
        st = 3
    else:
        st = 0
    return st, (b1[2], b1[3]), (b1[0], var_ref, b1[1]), sec


def test_the_vectorised_statement_is_the_literal_one():
    rng = np.random.RandomState(12); seen = set()
    base = rng.uniform(0, 255, (12, 14)); img = np.clip(np.kron(base, np.ones((4, 4))) + rng.normal(0, 5, (48, 56)), 0, 255).astype(np.uint8)
    lv = [img, img[::2, ::2].copy()]
    for i in range(120):
        l = int(rng.randint(-1, 3)); h, w = lv[l].shape if 0 <= l < 2 else (48, 56)
        x, y = int(rng.randint(-12, w + 12)), int(rng.randint(-12, h + 12)); radius = int(rng.choice([0, 1, 3, 8]))
        sx, sy = int(rng.randint(4, w - 3)), int(rng.randint(4, h - 3)); src = lv[l] if 0 <= l < 2 else img
        a = (src[sy - 4:sy + 4, sx - 4:sx + 4].reshape(64) if i % 3 else rng.randint(0, 256, 64)).astype(np.uint8)
        if i % 17 == 0:
            a = np.full(64, 9, np.uint8)
        args = (radius, int(rng.choice([1, 2, 3])), int(rng.choice([0, 4096, 147456])), int(rng.choice([0, 512, 920])), int(rng.choice([0, 700, 1000])))
        got = R.search_one(lv, x, y, l, a, *args)
        assert got == _slow(lv, x, y, l, a, *args), (i, x, y, l, args)
        seen.add(got[0])
    assert seen == {-1, 0, 1, 2, 3}
