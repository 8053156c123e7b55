"""One Levenberg-Marquardt step of the four per-frame pose optimisers, written from the measurement model alone.

Shares nothing with csrc/poseopt.hip or oracle/opt_oracle.c: the residuals are the three measurement models, the 2x6 pose Jacobian is a central
difference of e(exp(u) T) in np.longdouble (no analytic Jacobian anywhere in this file), the flow-coupled problems are solved as the UN-eliminated
(6 + 2 n) system with the flows as unknowns (the dense form), and only for large n with the 2x2 flow blocks eliminated in numpy (the eliminated
form; tests/test_pose_step_cpu.py shows the two agree before it relies on the second).

    one_step(problem)      the state after one accepted LM step of a problem with rounds=1, iters=[1,1,1,1], chi2_th=[1e30]*4
    as_one_step(problem)   that restriction of a problem dict
    edge_chi2(problem, T, flow)   info * |e|^2 per edge, the number the end-of-round classification compares with the threshold

Below them: the case builders and the order-stability helper the CPU and GPU tests of the pose optimisers share.
"""
import numpy as np

LD = np.longdouble
FD_STEP = 1e-7
DENSE_MAX_N = 257          # largest n the un-eliminated flow system is formed for

# D_step: the largest |one_step - oracle| over the case list of tests/test_pose_step_cpu.py (which asserts the measured value stays below these and prints
# it).  The GPU test allows 100 x as much (a 512-thread tree against a sequential loop).  Measured: pose 9.5e-12 (n = 3), flow 9.2e-13 (flow2cam at n = 3).
D_STEP_POSE = 1e-11
D_STEP_FLOW = 1e-12


# ---- SE(3), (omega, upsilon) ordering as problems.se3_exp -------------------------------------------------------------------------------------------------
def se3_exp(u):
    u = np.asarray(u, LD)
    w, v = u[:3], u[3:]
    th2 = w @ w
    th = np.sqrt(th2)
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)
    if th < 1e-3:              # Taylor series: the next terms are below 1e-29
        a = 1 - th2 / 6 + th2 * th2 / 120 - th2 ** 3 / 5040
        b = LD(1) / 2 - th2 / 24 + th2 * th2 / 720 - th2 ** 3 / 40320
        c = LD(1) / 6 - th2 / 120 + th2 * th2 / 5040 - th2 ** 3 / 362880
    else:
        a = np.sin(th) / th
        b = (1 - np.cos(th)) / th2
        c = (th - np.sin(th)) / (th2 * th)
    I = np.eye(3, dtype=LD)
    T = np.eye(4, dtype=LD)
    T[:3, :3] = I + a * O + b * (O @ O)
    T[:3, 3] = (I + b * O + c * (O @ O)) @ v
    return T


# ---- measurement models -----------------------------------------------------------------------------------------------------------------------------------
def residuals(p, T, f=None):
    """(n, 2) longdouble residuals of problem p at pose T (4x4) and, for the flow problems, flows f (n, 2)."""
    T = np.asarray(T, LD)
    obs = np.asarray(p["obs"], LD).reshape(-1, 2)
    fx, fy, cx, cy = LD(p["fx"]), LD(p["fy"]), LD(p["cx"]), LD(p["cy"])
    if p["mode"] == 1:                                             # back-project the last frame's pixel with its depth, carry it to the world
        d = np.asarray(p["depth"], LD).reshape(-1)
        Xl = np.stack([(obs[:, 0] - cx) * d / fx, (obs[:, 1] - cy) * d / fy, d], 1)
        Twl = np.asarray(p["Twl"], LD)
        X = Xl @ Twl[:3, :3].T + Twl[:3, 3]
    else:
        X = np.asarray(p["Xw"], LD).reshape(-1, 3)
    Y = X @ T[:3, :3].T + T[:3, 3]
    if p["mode"] == 2:                                             # obs - dehomogenised P T X
        P = np.asarray(p["P"], LD).reshape(3, 4)
        m = Y @ P[:, :3].T + P[:, 3]
        return obs - m[:, :2] / m[:, 2:3]
    pred = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1)
    if p["mode"] == 1:
        return (obs + np.asarray(f, LD).reshape(-1, 2)) - pred
    return obs - pred


def edge_chi2(p, T, flow=None):
    e = residuals(p, T, flow)
    return np.asarray(LD(p["info_edge"]) * (e * e).sum(1), np.float64)


def _robust(p, c2):
    """g2o's Huber on c2 = info |e|^2: (rho, rho') per edge."""
    rho, w = c2.copy(), np.ones_like(c2)
    if p["use_huber"]:
        delta = LD(p["huber_delta"])
        big = c2 > delta * delta
        s = np.sqrt(c2[big])
        rho[big] = 2 * s * delta - delta * delta
        w[big] = delta / s
    return rho, w


def _chi2(p, T, f):
    e = residuals(p, T, f)
    rho, _ = _robust(p, LD(p["info_edge"]) * (e * e).sum(1))
    chi = rho.sum()
    if p["mode"] == 1:
        r = np.asarray(f, LD) - np.asarray(p["flow0"], LD).reshape(-1, 2)
        chi += LD(p["info_prior"]) * (r * r).sum()
    return float(chi)


def _solve_refined(A, b):
    """float64 solve plus one correction from the residual formed in long double."""
    A64, b64 = np.asarray(A, np.float64), np.asarray(b, np.float64)
    x = np.linalg.solve(A64, b64).astype(LD)
    r = b - A @ x
    return x + np.linalg.solve(A64, np.asarray(r, np.float64)).astype(LD)


def as_one_step(p):
    q = dict(p)
    q.update(rounds=1, iters=[1, 1, 1, 1], chi2_th=[1e30] * 4)
    return q


def one_step(p, form=None):
    """T1, f1 after one LM step from (T_init, flow0), and the robust chi2 before and after.  form: "dense" / "eliminated" for the flow problems
    (default: dense up to DENSE_MAX_N points)."""
    n = p["n"]
    T0 = np.asarray(p["T_init"], LD).reshape(4, 4)
    flowm = p["mode"] == 1
    f0 = np.asarray(p["flow0"], LD).reshape(n, 2) if flowm else None
    e = residuals(p, T0, f0)
    J = np.empty((n, 2, 6), LD)
    h = LD(FD_STEP)
    for k in range(6):
        u = np.zeros(6, LD); u[k] = h
        J[:, :, k] = (residuals(p, se3_exp(u) @ T0, f0) - residuals(p, se3_exp(-u) @ T0, f0)) / (2 * h)
    info = LD(p["info_edge"])
    _, w = _robust(p, info * (e * e).sum(1))
    wo = w * info
    App = np.einsum("i,iak,ial->kl", wo, J, J)
    bp = -np.einsum("i,iak,ia->k", wo, J, e)
    if not flowm:
        lam = LD(1e-5) * np.abs(np.diag(App)).max()
        x = _solve_refined(App + lam * np.eye(6, dtype=LD), bp)
        xf = None
    else:
        ip = LD(p["info_prior"])
        r = f0 - np.asarray(p["flow0"], LD).reshape(n, 2)         # the prior's residual f - flow0 (zero at the start)
        dff = wo + ip                                             # the 2x2 flow blocks are (wo + info_prior) I: identity Jacobians of both edges
        bf = -wo[:, None] * e - ip * r
        Apf = wo[:, None, None] * np.transpose(J, (0, 2, 1))      # (n, 6, 2): wo J^T (de/df = I)
        lam = LD(1e-5) * max(np.abs(np.diag(App)).max(), np.abs(dff).max())
        if form is None:
            form = "dense" if n <= DENSE_MAX_N else "eliminated"
        if form == "dense":
            N = 6 + 2 * n
            A = np.zeros((N, N), LD); b = np.zeros(N, LD)
            A[:6, :6] = App; b[:6] = bp; b[6:] = bf.reshape(-1)
            for i in range(n):
                s = slice(6 + 2 * i, 8 + 2 * i)
                A[:6, s] = Apf[i]; A[s, :6] = Apf[i].T
                A[s, s] = dff[i] * np.eye(2, dtype=LD)
            x = _solve_refined(A + lam * np.eye(N, dtype=LD), b)
            xf = x[6:].reshape(n, 2); x = x[:6]
        else:
            dinv = 1 / (dff + lam)
            S = App + lam * np.eye(6, dtype=LD) - np.einsum("i,ika,ila->kl", dinv, Apf, Apf)
            bs = bp - np.einsum("i,ika,ia->k", dinv, Apf, bf)
            x = _solve_refined(S, bs)
            xf = dinv[:, None] * (bf - np.einsum("ika,k->ia", Apf, x))
    T1 = se3_exp(x) @ T0
    f1 = f0 + xf if flowm else None
    return dict(T=np.asarray(T1, np.float64), flow=np.asarray(f1, np.float64) if flowm else np.zeros((n, 2)),
                chi2_before=_chi2(p, T0, f0), chi2_after=_chi2(p, T1, f1))


# ---- the cases the CPU and GPU tests share ------------------------------------------------------------------------------------------------------------------
BUILDERS = ("new", "flow2cam", "flow2", "objmot")
EDGE_N = (3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025, 2049, 4096, 4097, 6000)
STEP_N = tuple(n for n in EDGE_N if n <= 1025)
OUTLIER_FRACS = (0.05, 0.5)
H_TRUE = (0.01, 0.03, -0.02, 0.4, 0.05, 0.2)
# seed of a case.  A seed must meet three input rules, all of them properties of the oracle and the numpy step alone (tests/test_pose_step_cpu.py asserts
# them): no edge's chi2 within 1e-6 relative of a round's threshold (order_stability asserts it too); the first LM trial of the one-step form accepted; and a
# verdict of "order-stable" from the three permutations must hold under the wide set of permutations as well (verdict_holds_widely).  The last rule is there
# because three permutations miss a count that flips one time in four with probability 0.42: such a case is a coin toss of the stop rule that lands in the
# exact group, where no implementation but the oracle itself could be expected to agree.  A case that fails a rule takes the next seed of default + 10000 j.
# The exceptions below all come from the third rule (flow2 at n = 3: chi2 ends near 1e-28 and the oracle gives 18 or 20 iterations over the six orders of
# three edges; objmot: 5 or 6 iterations in 50 / 150 of 200 permutations at n = 256).
SEED_EXCEPTIONS = {(3, 0.05): 11003, (3, 0.5): 511003, (63, 0.05): 11063, (255, 0.5): 511255, (256, 0.05): 11256, (512, 0.05): 11512}
WIDE_PERMUTATIONS = 24


def case_seed(n, outlier_frac):
    return SEED_EXCEPTIONS.get((n, outlier_frac), 1000 + n + (500000 if outlier_frac >= 0.5 else 0))


def scene_problems(P, n, seed, outlier_frac, noise_px=0.05, objmot_init="identity"):
    """The four problems over one synthetic scene of n points (P = vido_slam_amd.problems), and the truth: T_cur for the camera problems, H for objmot.
    outlier_frac is the scene's (the camera problems' matches); the object's points carry noise only and no robust kernel, as in the tracker, and its motion
    starts at the identity or, for the ground-truth test, at a perturbed H."""
    s = P.synth_pose_scene(n, seed=seed, noise_px=noise_px, outlier_frac=outlier_frac)
    rng = np.random.RandomState(seed + 7919)
    H = P.se3_exp(H_TRUE)
    fx, fy, cx, cy = s["K"]
    Xc = (s["Xw"] @ H[:3, :3].T + H[:3, 3]) @ s["T_cur"][:3, :3].T + s["T_cur"][:3, 3]
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * fx + cx, Xc[:, 1] / Xc[:, 2] * fy + cy], 1)
    if noise_px:
        obs = obs + rng.normal(0, noise_px, (n, 2))
    H_init = np.eye(4) if objmot_init == "identity" else P.se3_exp(rng.normal(0, 0.01, 6)) @ H
    probs = {
        "new": P.pose_problem_new(s["Xw"], s["uv_cur"], s["K"], s["T_init"]),
        "flow2cam": P.pose_problem_flow2cam(s["uv_last"], s["flow"], s["depth"], s["Twl"], s["K"], s["T_init"]),
        "flow2": P.pose_problem_flow2(s["uv_last"], s["flow"], s["depth"], s["Twl"], s["K"], s["T_init"]),
        "objmot": P.pose_problem_objmot(s["Xw"], obs, s["K"], s["T_cur"], H_init),
    }
    truth = {"new": s["T_cur"], "flow2cam": s["T_cur"], "flow2": s["T_cur"], "objmot": H}
    return probs, truth


def permuted(p, perm):
    q = dict(p)
    for k in ("Xw", "obs", "flow0", "depth"):
        if p.get(k) is not None:
            q[k] = np.ascontiguousarray(np.asarray(p[k])[perm])
    return q


def assert_clear_of_thresholds(oracle, p, label=""):
    """No edge's chi2 lies within 1e-6 relative of its round's threshold, in any round: the state a round ends in is the result of the same problem cut
    to that many rounds, and the classification's chi2 is edge_chi2 there (the errors the last accepted trial left, or those of a rejected trial a
    factor 2^45 in lambda away from it)."""
    for r in range(1, p["rounds"] + 1):
        q = dict(p); q["rounds"] = r
        res = oracle.pose_optimize(q)
        if p["n"] < 3:
            continue
        th = float(np.float32(p["chi2_th"][r - 1]))
        c = edge_chi2(p, res["T"], res["flow"])
        gap = np.abs(c - th).min() / th
        assert gap > 1e-6, "%s: an edge's chi2 is %.3g relative from the threshold of round %d: choose another seed" % (label, gap, r)


_VERDICTS = {}


def order_stability(oracle, p, key=None):
    """Runs the oracle on p and on three fixed permutations of its edges.  Returns (ref, stable, spread): the unpermuted result, whether lm_iterations, n_inliers and
    the permuted-back outlier flags agree on all four runs, and the largest pose difference between the runs.  Asserts the input rule of the exact
    flag comparison on all four."""
    if key is not None and key in _VERDICTS:
        return _VERDICTS[key]
    n = p["n"]
    ref = oracle.pose_optimize(p)
    assert_clear_of_thresholds(oracle, p, "%s unpermuted" % (key,))
    stable, spread = True, 0.0
    for k in (1, 2, 3):
        perm = np.random.RandomState(100 + k).permutation(n)
        q = permuted(p, perm)
        r = oracle.pose_optimize(q)
        assert_clear_of_thresholds(oracle, q, "%s permutation %d" % (key, k))
        back = np.zeros(n, bool); back[perm] = r["outlier"]
        stable = stable and r["lm_iterations"] == ref["lm_iterations"] and r["n_inliers"] == ref["n_inliers"] and np.array_equal(back, ref["outlier"])
        spread = max(spread, float(np.abs(r["T"] - ref["T"]).max()))
    out = (ref, stable, spread)
    if key is not None:
        _VERDICTS[key] = out
    return out


def wide_permutations(n):
    """every order of the edges but the given one up to n = 4, else WIDE_PERMUTATIONS fixed ones, the three of order_stability first"""
    if n <= 4:
        import itertools
        return [np.array(q) for q in itertools.permutations(range(n))][1:]
    return [np.random.RandomState(100 + k).permutation(n) for k in range(1, WIDE_PERMUTATIONS + 1)]


def verdict_holds_widely(oracle, p, ref):
    """the seeds' third input rule: the counts and flags of ref (the unpermuted oracle run) come out of every permutation of wide_permutations"""
    n = p["n"]
    for perm in wide_permutations(n):
        r = oracle.pose_optimize(permuted(p, perm))
        back = np.zeros(n, bool); back[perm] = r["outlier"]
        if not (r["lm_iterations"] == ref["lm_iterations"] and r["n_inliers"] == ref["n_inliers"] and np.array_equal(back, ref["outlier"])):
            return False
    return True
