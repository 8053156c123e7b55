"""GPU parity of the seeded P3P-RANSAC (csrc/pnp.hip) at the edges of its launch geometry: k_pnp_solve runs 64 hypotheses per workgroup, k_pnp_score scores
4 per workgroup with the points strided by 256, k_pnp_select replays the sequential bookkeeping.  Rule of test_pnp_ransac_matches_oracle: pose within 1e-6,
masks exact outside the 1e-6 px^2 band round the threshold — and every seed here is one for which the oracle puts NO point in that band (asserted on the
CPU in every case), so the masks are simply equal.

Measured on an MI355X (profiles/r18/pose_pnp_edges.txt): over all 61 comparisons of this file the GPU's pose differs from the oracle's by 2.7e-14 at worst (bound
1e-6) with equal masks and counts.  Ground truth (zero noise, no outliers, inputs rounded to float32): the oracle's own error is 4.8e-8 at n = 100 and 2.9e-8 at
n = 1000 (ORACLE_TRUTH_ERR), the tolerance 10 x that (the GPU's pose lies within 3e-14 of the oracle's there).
"""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = (520.0, 515.0, 320.0, 240.0)
THR = 0.4
BAND = 1e-6
NS = (4, 5, 6, 7, 255, 256, 257, 1000)
ITERS = (1, 3, 4, 5, 63, 64, 65, 501)
# the oracle's error against the true pose with exact inputs rounded to float32 (n = 100, n = 1000), measured on the CPU; the assertion below re-measures it
ORACLE_TRUTH_ERR = {100: 4.8e-8, 1000: 2.9e-8}
# seeds that replace the default where the default puts a point of the winning model inside the band (none has been needed)
SEED_EXCEPTIONS = {}
CONF_SEED = 80


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context()
    yield c
    c.close()


def case_seed(n, it):
    return SEED_EXCEPTIONS.get((n, it), 1000 * n + it)


def reproj2(T, X, x):
    """squared reprojection error of the float32 points as csrc/pnp.hip's reproj2 states it (1e30 behind the camera)"""
    X = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3); x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 2)
    Xc = X @ T[:3, :3].T + T[:3, 3]
    ok = Xc[:, 2] > 1e-9
    z = np.where(ok, Xc[:, 2], 1.0)
    e2 = (K[0] * Xc[:, 0] / z + K[2] - x[:, 0]) ** 2 + (K[1] * Xc[:, 1] / z + K[3] - x[:, 1]) ** 2
    return np.where(ok, e2, 1e30)


def check(vido, oracle, ctx, X, x, seed, max_iters=500, conf=0.98, label=None, tol=1e-6):
    """one problem on the GPU against the oracle: the input rule (no point in the band), then equal winners: pose, mask and count"""
    Tr, maskr, cntr, Tm = oracle.pnp_ransac(X, x, K, max_iters=max_iters, thr=THR, conf=conf, seed=seed, with_ransac_model=True)
    if cntr:
        e2 = reproj2(Tm, X, x)
        assert not (np.abs(e2 - THR * THR) <= BAND).any(), ("a point lies in the band: choose another seed", label, seed)
        assert np.array_equal(e2 <= THR * THR, maskr)
    T, mask, cnt = vido.pnp_ransac(ctx, X, x, K, max_iters=max_iters, reproj_err=THR, confidence=conf, seed=seed)
    assert np.isfinite(T).all()
    assert cnt == cntr and np.array_equal(mask, maskr), (label, cnt, cntr)
    print("  %s: %d inliers, pose difference from the oracle %.2e" % (label, cnt, np.abs(T - Tr).max()))
    assert np.abs(T - Tr).max() < tol, (label, np.abs(T - Tr).max())
    return T, mask, cnt


def scene(vido, n, seed, outl=0.2, noise=0.05):
    s = vido.problems.synth_pose_scene(n, seed=seed, noise_px=noise, outlier_frac=outl)
    return s["Xw"], s["uv_cur"], s


@pytest.mark.parametrize("n", NS)
def test_point_count_by_iteration_grid(vido, oracle, ctx, n):
    """n round the 256-point stride of the scoring and select loops (and the smallest a 4-point sample can be drawn from) x iteration counts round the 4 hypotheses
    of a scoring workgroup and the 64 of a solving one.  The winners differ over the grid (printed), so a hypothesis scored or skipped wrongly shows."""
    winners = []
    for it in ITERS:
        seed = case_seed(n, it)
        X, x, _ = scene(vido, n, seed)
        _, _, cnt = check(vido, oracle, ctx, X, x, seed, max_iters=it, label=(n, it))
        winners.append(cnt)
    print("n = %d: inliers at max_iters %s = %s" % (n, ITERS, winners))
    if n >= 255:
        assert len(set(winners)) > 1 and max(winners) > 0.5 * n


@pytest.mark.parametrize("conf", [0.5, 0.98, 0.999999])
def test_confidence_sets_the_iteration_cap(vido, oracle, ctx, conf):
    """50 % outliers at n = 500: ransac_update_iters cuts the loop at a confidence-dependent iteration; a different cap would crown a different hypothesis."""
    X, x, _ = scene(vido, 500, CONF_SEED, outl=0.5)
    _, _, cnt = check(vido, oracle, ctx, X, x, CONF_SEED, conf=conf, label=("conf", conf))
    assert cnt > 100


def test_confidences_pick_different_winners(oracle, vido):
    """the three confidences are a real test of the cap: on one input the oracle's winner changes with the confidence"""
    X, x, _ = scene(vido, 500, CONF_SEED, outl=0.5)
    models = [oracle.pnp_ransac(X, x, K, conf=c, seed=CONF_SEED, with_ransac_model=True)[3] for c in (0.5, 0.98, 0.999999)]
    assert not np.array_equal(models[0], models[1]) and not np.array_equal(models[1], models[2])


def _batch(vido, ctx, probs, seeds, max_iters=500):
    m = len(probs)
    X = [np.ascontiguousarray(p[0], np.float32).reshape(-1, 3) for p in probs]; x = [np.ascontiguousarray(p[1], np.float32).reshape(-1, 2) for p in probs]
    ns = np.array([len(a) for a in X], np.int32); seeds = np.asarray(seeds, np.uint64)
    T = np.zeros((m, 16)); masks = [np.zeros(max(n, 1), np.uint8) for n in ns]; cnt = np.zeros(m, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    p3 = (C.c_void_p * m)(*[a.ctypes.data if len(a) else None for a in X]); p2 = (C.c_void_p * m)(*[a.ctypes.data if len(a) else None for a in x])
    pm = (C.c_void_p * m)(*[k.ctypes.data for k in masks])
    ctx._check(ctx.lib.vido_pnp_ransac_batch(ctx.h, m, p3, p2, vp(ns), C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), max_iters, C.c_double(THR),
                                             C.c_double(0.98), vp(seeds), vp(T), pm, vp(cnt)))
    return [(T[i].reshape(4, 4), masks[i][:ns[i]].astype(bool), int(cnt[i])) for i in range(m)]


def test_batch_of_forty_equals_single_calls(vido, ctx):
    rng = np.random.RandomState(5)
    ns = rng.choice([0, 1, 2, 3, 4, 7, 300, 1200], 40)
    ns[:8] = [0, 1, 2, 3, 4, 7, 300, 1200]                      # every size at least once
    probs = [scene(vido, int(n), 200 + i)[:2] for i, n in enumerate(ns)]
    seeds = np.arange(40) + 900
    got = _batch(vido, ctx, probs, seeds)
    for i, (X, x) in enumerate(probs):
        Ti, mi, ci = vido.pnp_ransac(ctx, X, x, K, seed=int(seeds[i]))
        assert np.array_equal(got[i][0], Ti) and got[i][2] == ci and np.array_equal(got[i][1], mi), (i, ns[i])
        if ns[i] < 4:
            assert ci == 0 and np.array_equal(Ti, np.eye(4)) and not mi.any()
    assert sum(g[2] > 0 for g in got) >= 10


def test_small_large_small_on_one_context(vido, ctx):
    """the device block grows at the large call and is reused by the small one after it: each call equals the same call on a fresh context"""
    calls = [(scene(vido, n, 300 + i)[:2], 40 + i) for i, n in enumerate((5, 2500, 6, 257))]
    got = [vido.pnp_ransac(ctx, X, x, K, seed=s) for (X, x), s in calls]
    for ((X, x), s), g in zip(calls, got):
        fresh = vido.Context()
        try:
            r = vido.pnp_ransac(fresh, X, x, K, seed=s)
        finally:
            fresh.close()
        assert np.array_equal(r[0], g[0]) and np.array_equal(r[1], g[1]) and r[2] == g[2]


def test_degenerate_inputs_match_oracle(vido, oracle, ctx):
    rng = np.random.RandomState(3)
    proj = lambda X: np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)
    # eight copies of one point: every triangle has zero sides
    X = np.tile([[0.5, -0.25, 6.0]], (8, 1)); T, mask, cnt = check(vido, oracle, ctx, X, proj(X), 5, label="copies")
    assert cnt == 0 and np.array_equal(T, np.eye(4))
    # 30 collinear points, exact (binary fractions): the triangle of every sample has no area
    t = (np.arange(30) - 15)[:, None] / 8.0; X = np.array([[0.25, 0.5, 8.0]]) + t * np.array([[1.0, 0.5, 0.75]])
    T, mask, cnt = check(vido, oracle, ctx, X, proj(X), 6, label="collinear")
    assert cnt == 0
    # 50 coplanar points, exact (coordinates on a binary grid: the float32 inputs are the exact ones), seen from the identity
    X = np.stack([rng.randint(-64, 65, 50) / 16.0, rng.randint(-48, 49, 50) / 16.0, np.full(50, 8.0)], 1)
    T, mask, cnt = check(vido, oracle, ctx, X, proj(X), 7, label="coplanar")
    assert cnt == 50 and np.abs(T - np.eye(4)).max() < 5e-7
    # half the points behind the camera (their error is 1e30 under every model)
    X, x, s = scene(vido, 200, 9, outl=0.0)
    X = X.copy(); back = np.arange(200) % 2 == 1
    Tcw = s["T_cur"]; Xc = X @ Tcw[:3, :3].T + Tcw[:3, 3]; Xc[back, 2] *= -1
    Twc = np.linalg.inv(Tcw); X = Xc @ Twc[:3, :3].T + Twc[:3, 3]
    T, mask, cnt = check(vido, oracle, ctx, X, x, 8, label="behind")
    assert cnt > 80 and not mask[back].any() and np.abs(T - Tcw).max() < 0.05


@pytest.mark.parametrize("n", [100, 1000])
def test_ground_truth(vido, oracle, ctx, n):
    """zero noise, no outliers: the pose is the true one, to 10 x the oracle's own error on the same float32-rounded inputs"""
    seed = case_seed(n, 0)
    X, x, s = scene(vido, n, seed, outl=0.0, noise=0.0)
    Tr = oracle.pnp_ransac(X, x, K, seed=seed)[0]
    err = np.abs(Tr - s["T_cur"]).max()
    print("n = %d: oracle's error against the truth %.3e" % (n, err))
    assert err <= ORACLE_TRUTH_ERR[n] * 1.0000001, "re-measure ORACLE_TRUTH_ERR"
    T, mask, cnt = check(vido, oracle, ctx, X, x, seed, label=("truth", n))
    assert cnt == n and mask.all()
    assert np.abs(T - s["T_cur"]).max() <= 10 * ORACLE_TRUTH_ERR[n]
