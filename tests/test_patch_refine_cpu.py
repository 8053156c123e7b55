"""CPU: the numpy / Python-integer statement of vido_orb_patch_refine (tests/refimpl/patch_refine_np.py) against a plain float64 Gauss-Newton on the same model, on the
constructed patches whose answer follows from the definition alone, and against its own int64 bounds.  No GPU; tests/test_patch_refine_gpu.py holds the kernel to this
statement bit for bit."""
import numpy as np
import pytest

from refimpl import patch_refine_np as R


def _smooth(seed, h=48, w=56, cell=4):
    """byte image of full contrast with structure `cell` px wide (random grid values, bilinearly upsampled)"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 256, (h // cell + 2, w // cell + 2)).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w] / float(cell)
    y0, x0 = yy.astype(int), xx.astype(int); ay, ax = yy - y0, xx - x0
    v = (1 - ay) * (1 - ax) * g[y0, x0] + (1 - ay) * ax * g[y0, x0 + 1] + ay * (1 - ax) * g[y0 + 1, x0] + ay * ax * g[y0 + 1, x0 + 1]
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _gauss_newton64(L, x, y, T, max_steps=40):
    """The same model in float64 with nothing rounded: bilinear image, template gradients (twice the central difference), zero-mean (bias) normal equations, the
    inverse-compositional step -2 H^-1 b in px.  Returns (p in px, converged, largest |p| met, contraction: the last |step| ratio)."""
    T = T.reshape(8, 8).astype(np.float64); L = L.astype(np.float64)
    gx = (T[1:7, 2:8] - T[1:7, 0:6]).ravel(); gy = (T[2:8, 1:7] - T[0:6, 1:7]).ravel(); t = T[1:7, 1:7].ravel()
    G = np.stack([gx - gx.mean(), gy - gy.mean()], 1); H = G.T @ G
    p = np.zeros(2); far = 0.0; last = None; rate = 0.0
    for _ in range(max_steps):
        X = x - 4 + np.arange(1, 7) + p[0]; Y = y - 4 + np.arange(1, 7) + p[1]
        ix, iy = np.floor(X).astype(int), np.floor(Y).astype(int)[:, None]; fx, fy = X - np.floor(X), (Y - np.floor(Y))[:, None]
        I = ((1 - fx) * (1 - fy) * L[iy, ix] + fx * (1 - fy) * L[iy, ix + 1] + (1 - fx) * fy * L[iy + 1, ix] + fx * fy * L[iy + 1, ix + 1]).ravel()
        e = I - t
        d = -2.0 * np.linalg.solve(H, G.T @ (e - e.mean()))
        p = p + d; far = max(far, float(np.abs(p).max()))
        nd = float(np.hypot(*d))
        if far > 1.4:
            return p, False, far, 1.0
        if last is not None and last > 0:
            rate = nd / last
        last = nd
        if nd < 1e-9:
            return p, True, far, rate
    return p, False, far, rate


def test_agrees_with_float64_gauss_newton_on_well_conditioned_patches():
    """Well conditioned: the float64 iteration converges inside the window and the integer one ends by a zero step before its 8 steps run out.  Then both sit at the
    minimum of the same cost: the integer steps stop once |step| < 1/512 px and e is rounded to 1/256 grey level, which the bound of 2/256 px covers."""
    rng = np.random.RandomState(3); n_ok = 0; worst = 0.0
    for k in range(120):
        L = _smooth(100 + k % 6)
        x, y = int(rng.randint(12, 44)), int(rng.randint(12, 36))
        px, py = (int(v) for v in rng.randint(-200, 201, 2))
        T = R.resample(L, x, y, px, py)
        st, q8, cost, steps = R.refine_one([L], x, y, 0, T, 8, 384, 0)
        p, conv, far, rate = _gauss_newton64(L, x, y, T)
        if st != 0 or not conv or steps == 8:
            continue
        n_ok += 1
        d = max(abs(q8[0] / 256.0 - p[0]), abs(q8[1] / 256.0 - p[1])); worst = max(worst, d)
        assert d <= 2.0 / 256.0, (k, q8, p, steps)
        assert cost[1] <= cost[0]
    print("float64 Gauss-Newton: %d of 120 well conditioned, largest difference %.5f px" % (n_ok, worst))
    assert n_ok >= 60


def test_constructed_patches():
    cons = R.constructed()
    assert {"flat", "vertical_edge", "checker", "ramp", "leaves_window", "known_offset"} <= set(cons)
    seen = set()
    for name, c in cons.items():
        st, q8, cost, steps = R.refine_one([c["img"]], 8, 8, 0, c["ref"], c["iters"], c["max_shift_q8"], c["min_eig"])
        seen.add(st)
        if c["status"] is not None:
            assert st == c["status"], name
        if st in (2, 3):
            assert q8 == (0, 0) and cost[0] == cost[1]
        if st == 2:
            assert cost == (0, 0) and steps == 0
        if "steps" in c:
            assert steps == c["steps"], name
        if name == "known_offset":
            assert max(abs(q8[0] - c["q8"][0]), abs(q8[1] - c["q8"][1])) <= 1 and cost[1] < cost[0], (q8, cost)
        elif "q8" in c:
            assert q8 == c["q8"], name
    assert {0, 2, 3} <= seen
    det, tr = R.hessian(cons["vertical_edge"]["ref"])[7:9]
    assert det == 0 and tr > 0                                                      # an edge: one eigenvalue only
    assert R.hessian(cons["ramp"]["ref"])[4:7] == (0, 0, 0) and R.hessian(cons["flat"]["ref"])[4:7] == (0, 0, 0)


def test_int64_bounds_on_the_checker():
    """The docstring's bounds, and how close the 2-px checker comes to them: H and det exactly at the bound, |e| at 65 280 against its inverse, and every product of the
    step inside int64 with the shifted checker, whose error is in step with the gradient."""
    E, G, N = 65280, 255, R.N
    B_b, B_h, B_cost = N * N * G * E, N * N * G * G, N * N * E * E
    assert B_b < 2 ** 34.4 and B_h < 2 ** 26.4 and B_h * B_h < 2 ** 53 and 2 * (2 * B_h * B_b) < 2 ** 62.7 < 2 ** 63 - 1 and B_cost < 2 ** 42.4
    m = 2 ** 31 - 1
    assert m * 2 * B_h < 2 ** 63 and B_h * B_h + m * m < 2 ** 63                    # the gate's terms at the largest min_eig
    cons = R.constructed()
    hxx, hyy, hxy, det, tr = R.hessian(cons["checker"]["ref"])[4:9]
    assert hxx == hyy == B_h and hxy == 0 and det == B_h * B_h
    big = {}
    for name in ("checker", "checker_inverse", "checker_shifted"):
        c = cons[name]
        for iters in (1, 8):
            for shift in (0, 256, 512):
                t = {}
                R.refine_one([c["img"]], 8, 8, 0, c["ref"], iters, shift, 0, t)
                for k, v in t.items():
                    if k != "path":
                        big[k] = max(big.get(k, 0), v)
    print("largest on the checkers: " + "  ".join("%s 2^%.1f" % (k, np.log2(max(v, 1))) for k, v in sorted(big.items())))
    assert big["max_e"] == E and big["max_h"] == B_h and big["max_det"] == B_h * B_h
    assert 0 < big["max_b"] <= B_b and big["max_cost"] <= B_cost and big["max_cost"] > 2 ** 40
    assert 2 ** 55 < big["max_2num"] <= 4 * B_h * B_b < 2 ** 63


def test_every_status_the_gate_and_the_parameter_refusals():
    L = _smooth(5); T = R.resample(L, 20, 20, 40, -30)
    assert R.refine_one([L], 20, 20, 0, T, 6, 384, 0)[0] == 0
    assert R.refine_one([L], 20, 20, 1, T, 6, 384, 0)[0] == -1 and R.refine_one([L], 20, 20, -1, T, 6, 384, 0)[0] == -1
    h, w = L.shape
    for shift, C in ((0, 0), (1, 1), (255, 1), (256, 1), (257, 2), (384, 2), (512, 2)):   # both sides of every border of rule 1
        for x, y, ok in ((3 + C, 20, True), (2 + C, 20, False), (w - 4 - C, 20, True), (w - 3 - C, 20, False), (20, 3 + C, True), (20, 2 + C, False), (20, h - 4 - C, True), (20, h - 3 - C, False)):
            assert (R.refine_one([L], x, y, 0, T, 1, shift, 0)[0] != -1) == ok, (shift, x, y)
    assert R.refine_one([L], 1 << 31, 20, 0, T, 1, 0, 0)[0] == -1 and R.refine_one([L], -(1 << 31), 20, 0, T, 1, 0, 0)[0] == -1
    # the gate is the smaller eigenvalue, compared without a root
    hxx, hyy, hxy, det, tr = R.hessian(T)[4:9]
    lam = (tr - np.sqrt(float(tr) ** 2 - 4.0 * det)) / 2.0
    assert R.refine_one([L], 20, 20, 0, T, 6, 384, int(lam) - 1)[0] == 0 and R.refine_one([L], 20, 20, 0, T, 6, 384, int(lam) + 2)[0] == 2
    assert R.refine_one([L], 20, 20, 0, T, 6, 384, 2 ** 31 - 1)[0] == 2
    # a template 1.2 px away: max_shift_q8 0 and 256 give it up (the second step passes 256), 384 holds it and ends within 1/16 px (the patch is rounded to bytes)
    T2 = R.resample(L, 20, 20, 307, 0)
    assert R.refine_one([L], 20, 20, 0, T2, 6, 0, 0)[0] == 3 and R.refine_one([L], 20, 20, 0, T2, 6, 256, 0)[::3] == (3, 2)
    st, q8, cost, steps = R.refine_one([L], 20, 20, 0, T2, 8, 384, 0)
    assert st == 0 and abs(q8[0] - 307) <= 16 and abs(q8[1]) <= 16 and steps >= 2 and cost[1] < cost[0]
    assert R.rdiv(5, 2) == 3 and R.rdiv(-5, 2) == -3 and R.rdiv(4, 3) == 1 and R.rdiv(-7, 3) == -2 and R.rdiv(0, 9) == 0 and R.rdiv(1, 3) == 0
    for bad in ((0, 0, 0), (9, 0, 0), (1, -1, 0), (1, 513, 0), (1, 0, -1)):
        with pytest.raises(ValueError):
            R.patch_refine([L], np.zeros((0, 3)), np.zeros((0, 64)), *bad)
    q8, cost, it, st, stats = R.patch_refine([L], [(20, 20, 0), (20, 20, 7), (0, 0, 0)], np.stack([T, T, T]), 6, 384, 0)
    assert st.tolist() == [0, -1, -1] and stats.tolist() == [1, 0, 0, 2] and cost.dtype == np.int64 and q8.dtype == np.int32
