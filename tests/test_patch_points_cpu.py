"""CPU: the numpy / Python-integer statement of vido_orb_patch_points (tests/refimpl/patch_points_np.py) against a direct float64 ZNCC and on the constructed patches
whose sums and verdicts are known in closed form.  No GPU; tests/test_patch_points_gpu.py holds the kernel to this statement bit for bit."""
import numpy as np
import pytest

from refimpl import patch_points_np as R
from refimpl.patch_points_np import constructed


def _zncc64(a, b):
    a = a.astype(np.float64); b = b.astype(np.float64)
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return None if den == 0 else float((da * db).sum() / den)


def test_verdicts_agree_with_float64_zncc():
    """4000 random pairs (independent, correlated with noise of several strengths, low-contrast): the sums are those of the definition, and the integer verdict is the
    float64 one wherever the float value is further than 1e-9 from the threshold."""
    rng = np.random.RandomState(11)
    n_dec = 0; seen = set()
    for i in range(4000):
        a = rng.randint(0, 256, 64)
        kind = i % 4
        if kind == 0:
            b = rng.randint(0, 256, 64)
        elif kind == 1:
            b = np.clip(a + rng.normal(0, (2, 10, 40, 90)[(i // 4) % 4], 64), 0, 255)
        elif kind == 2:
            a = 100 + rng.randint(0, 4, 64); b = 100 + rng.randint(0, 4, 64)
        else:
            b = np.clip(0.5 * a + 60 + rng.normal(0, 5, 64), 0, 255)
        a = a.astype(np.uint8); b = np.rint(b).astype(np.uint8)
        cov, vr, vc = R.sums(a, b)
        A = a.astype(np.int64); B = b.astype(np.int64)
        assert (cov, vr, vc) == (int(64 * (A * B).sum() - A.sum() * B.sum()), int(64 * (A * A).sum() - A.sum() ** 2), int(64 * (B * B).sum() - B.sum() ** 2))
        z = _zncc64(a, b)
        for q in (0, 1, 512, 920, 1024):
            for min_var in (0, 4096, 147456):
                st = R.verdict(cov, vr, vc, min_var, q)
                seen.add(st)
                if vr < min_var or vc < min_var:
                    assert st == 2
                    continue
                if z is None:                             # a constant patch with min_var = 0: cov = 0, rejected
                    assert st == 1
                    continue
                if abs(z - q / 1024.0) <= 1e-9 or abs(z) <= 1e-9:
                    continue
                n_dec += 1
                assert st == (0 if (z > 0 and z >= q / 1024.0) else 1), (i, q, min_var, z, st)
    assert n_dec > 30000 and seen == {0, 1, 2}


def test_identical_patches_are_the_equality_case():
    C = constructed()
    for name in ("identical", "checker"):
        a, b = C[name]
        cov, vr, vc = R.sums(a, b)
        assert cov == vr == vc and cov * cov == vr * vc and cov > 0
        assert R.verdict(cov, vr, vc, 0, 1024) == 0      # cov^2 2^20 == 1024^2 var var: equality accepts
        assert R.verdict(cov, vr, vc, vr, 1024) == 0 and R.verdict(cov, vr, vc, vr + 1, 1024) == 2
    a, b = C["gain_offset"]                               # b = a + 100: ZNCC 1 exactly, another equality
    cov, vr, vc = R.sums(a, b)
    assert cov * cov == vr * vc and R.verdict(cov, vr, vc, 1, 1024) == 0


def test_inverse_is_rejected_at_threshold_zero():
    C = constructed()
    for name in ("inverse", "checker_inverse"):
        cov, vr, vc = R.sums(*C[name])
        assert cov < 0 and cov == -vr and vr == vc
        for q in (0, 1, 512, 1024):
            assert R.verdict(cov, vr, vc, 0, q) == 1


def test_white_against_white():
    cov, vr, vc = R.sums(*constructed()["white"])
    assert (cov, vr, vc) == (0, 0, 0)
    assert R.verdict(cov, vr, vc, 1, 0) == 2
    assert R.verdict(cov, vr, vc, 0, 0) == 1              # cov = 0 is not > 0
    cov, vr, vc = R.sums(*constructed()["flat_vs_random"])
    assert cov == 0 and vr == 0 and vc > 0 and R.verdict(cov, vr, vc, 0, 0) == 1 and R.verdict(cov, vr, vc, 1, 0) == 2


def test_checkerboard_is_the_maximum():
    a, b = constructed()["checker"]
    cov, vr, vc = R.sums(a, b)
    assert cov == vr == vc == 66585600 == R.VAR_MAX < 2 ** 31
    assert cov * cov * 1024 * 1024 > 2 ** 64              # the comparison really needs more than 64 bits
    rng = np.random.RandomState(3)
    for _ in range(2000):                                 # no patch of bytes exceeds it
        p = np.where(rng.uniform(size=64) < rng.uniform(0.3, 0.7), 255, 0).astype(np.uint8)
        assert R.sums(p, p)[1] <= R.VAR_MAX


def test_take_and_invalid_points():
    rng = np.random.RandomState(5)
    lv = [rng.randint(0, 256, (40, 50)).astype(np.uint8), rng.randint(0, 256, (20, 31)).astype(np.uint8)]
    xyl = np.array([(4, 4, 0), (46, 36, 0), (3, 4, 0), (4, 3, 0), (47, 36, 0), (46, 37, 0), (27, 16, 1), (28, 16, 1), (10, 10, 2), (10, 10, -1), (-5, 10, 0), (1 << 30, 10, 0)])
    ref = rng.randint(0, 256, (len(xyl), 64)).astype(np.uint8)
    patch, sm, st = R.patch_points(lv, xyl, ref, 0, 0)
    want_valid = np.array([1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0], bool)
    assert np.array_equal(st >= 0, want_valid)
    assert np.array_equal(patch[0], lv[0][0:8, 0:8].reshape(64)) and np.array_equal(patch[1], lv[0][32:40, 42:50].reshape(64)) and np.array_equal(patch[6], lv[1][12:20, 23:31].reshape(64))
    assert not patch[~want_valid].any() and not sm[~want_valid].any() and np.all(st[~want_valid] == -1)
    p2, none1, none2 = R.patch_points(lv, xyl)
    assert none1 is None and none2 is None and np.array_equal(p2, patch)
    with pytest.raises(ValueError):
        R.verdict(1, 1, 1, -1, 0)
    with pytest.raises(ValueError):
        R.verdict(1, 1, 1, 0, 1025)
