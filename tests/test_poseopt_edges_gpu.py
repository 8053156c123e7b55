"""GPU: k_pose_opt (csrc/poseopt.hip) at the edges of its launch geometry.  The point counts come from the code: the width of a single workgroup
nt = max(64, roundup64(ceil(n / 4))) <= 512 changes at 256 -> 257, the cluster size G = min(8, ceil(n / 512)) at 512 -> 513, 1024 -> 1025, ..., above 4096 a
cluster thread carries more than one edge; a batch is cut into launches of at most 64 workgroups, the exchange areas are reallocated when a batch grows, and the
epoch tags carry over from launch to launch on one context.

(a) against the C oracle, under the order-stability rule: lm_iterations (and with it everything compared exactly) is only asserted where the oracle itself
    gives the same counts and flags under three permutations of its edges (tests/refimpl/pose_step_np.order_stability; table in test_pose_step_cpu.py);
    all other cases: pose 1e-9 relative, chi2 and flows 1e-6, outlier flags exact.  Every seed is one for which no edge's chi2 lies within 1e-6 relative of a
    round's threshold in any of the four oracle runs (asserted), and for which a verdict of order-stable is not overturned by a wider set of permutations
    (all orders up to n = 4, else 24; asserted on the CPU by test_pose_step_cpu.py, see SEEDS below).
(b) one LM step against the independent numpy reference: |T - T1| <= 100 x D_step = 1e-9, |flow - f1| <= 1e-10 (D_step 1e-11 / 1e-12 recorded in
    pose_step_np.py, 9.5e-12 / 9.2e-13 measured).
(c) ground truth in all four modes, zero noise: tolerance 100 x the oracle's own worst error on the same inputs (ORACLE_TRUTH_ERR).
(d)-(h) batch invariance, launch splitting, state growth and reuse, small and hopeless inputs, refused inputs: bit for bit.

MEASURED on an MI355X (profiles/r18/pose_pnp_edges.txt):
  (a) worst pose difference from the oracle: 3.5e-10 in the order-stable group (123 cases; objmot, n = 255; bound 1e-4), 2.4e-10 in the tolerance group (21 cases;
      objmot, n = 512; bound 1e-9).  Everything but objmot agrees to 2.1e-12 or better.  The oracle's own spread under the three permutations is 6.3e-10 (objmot,
      n = 64; 5.9e-12 for the other kinds).  In the tolerance group lm_iterations differs in 16 of the 21 cases (e.g. 58 against 49, flow2cam at n = 3).
  (b) worst difference from one_step(): pose 9.5e-12 (n = 3), flow 9.2e-13: the GPU sits on the oracle, D_step is all of it.
  (c) the oracle's worst error against the truth 3.4e-10 (pose; objmot, n = 3) and 1.6e-9 (flow; flow2cam, n = 1024); the GPU's 3.4e-10 and 1.6e-9.

SEEDS.  The stop rule compares the chi2 of the last trial with the one before; once the gain is below the rounding of chi2 the iteration count is a coin toss, and
the kernel (sums over a wave tree, Schur totals subtracted after summing, (2 rho - 1)^3 by multiplication where the oracle calls pow()) is one more rounding of the
same algorithm.  Three permutations miss a count that flips one time in four with probability 0.42, and at the default seeds they did: they called order-stable
flow2 at n = 3 (the oracle itself: 18 iterations under five of the six orders of three edges, 20 under the sixth, chi2 3e-28; the GPU 17) and objmot at n = 256
(the oracle: 6 in 150 and 5 in 50 of 200 permutations; the GPU 5).  Such a case is not one the exact group can hold, and the helper's verdict is the only thing
that may move a case, so the input is changed, as for the threshold band: a seed is admitted only if every verdict of order-stable on its four problems also
holds under all orders of the edges (n <= 4) or 24 permutations (pose_step_np.verdict_holds_widely).  The rule reads the oracle alone, never the kernel; it is
asserted by test_pose_step_cpu.test_order_stability_table and replaced six default seeds (pose_step_np.SEED_EXCEPTIONS).  The verdict still comes from the three
permutations.
"""
import numpy as np
import pytest

from refimpl import pose_step_np as R

pytestmark = pytest.mark.gpu

# (c): the oracle's worst error against the truth over all sizes and the four modes with zero noise (pose, flow), measured on the CPU; re-measured by the test
ORACLE_TRUTH_ERR = (3.4e-10, 1.6e-9)


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.fixture(scope="module")
def P(vido):
    return vido.problems


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=640, height=480, max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def opt(vido, ctx):
    return vido.Optimizer(ctx)


def on_fresh_context(vido, call):
    c = vido.Context(width=640, height=480, max_batch=1)
    try:
        return call(vido.Optimizer(c))
    finally:
        c.close()


def same_bits(a, b):
    return (np.array_equal(a["T"], b["T"]) and np.array_equal(a["outlier"], b["outlier"]) and np.array_equal(a["flow"], b["flow"]) and
            a["n_inliers"] == b["n_inliers"] and a["lm_iterations"] == b["lm_iterations"] and a["chi2_final"] == b["chi2_final"])


def capped(p, iters=20):
    q = dict(p); q["iters"] = [iters] * 4
    return q


def compare_with_oracle(got, ref, stable, pr, label):
    """the rule of (a); returns the pose difference"""
    d = rel(got["T"], ref["T"])
    assert np.isfinite(got["T"]).all() and np.isfinite(got["flow"]).all(), label
    if stable:                                                       # exactly what test_four_optimisers_match_oracle asserts
        assert d < 1e-4, (label, d)
        assert got["lm_iterations"] == ref["lm_iterations"], (label, got["lm_iterations"], ref["lm_iterations"])
        assert got["n_inliers"] == ref["n_inliers"] and np.array_equal(got["outlier"], ref["outlier"]), label
        assert abs(got["chi2_final"] - ref["chi2_final"]) <= 1e-6 * max(1.0, ref["chi2_final"]), label
        if pr["mode"] == 1:
            assert np.abs(got["flow"] - ref["flow"]).max() < 1e-6, label
    else:
        assert d < 1e-9, (label, d)
        assert abs(got["chi2_final"] - ref["chi2_final"]) <= 1e-6 * max(1.0, ref["chi2_final"]), label
        assert np.abs(got["flow"] - ref["flow"]).max() < 1e-6, label
        assert np.array_equal(got["outlier"], ref["outlier"]) and got["n_inliers"] == ref["n_inliers"], label
    return d


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.EDGE_N)
def test_edge_sizes_match_oracle(P, oracle, opt, n):
    worst, failed = 0.0, []
    for of in R.OUTLIER_FRACS:
        probs, _ = R.scene_problems(P, n, R.case_seed(n, of), of)
        for name in R.BUILDERS:
            ref, stable, _ = R.order_stability(oracle, probs[name], (name, n, of))
            got = opt.pose_optimize(probs[name])
            print("  (a) %-8s n = %4d outliers %.2f: %-12s lm_iterations gpu %3d oracle %3d, pose difference %.2e" % (name, n, of, "order-stable" if stable else "NOT stable",
                                                                                                                      got["lm_iterations"], ref["lm_iterations"], rel(got["T"], ref["T"])))
            try:                                                     # (every case of this size is compared and printed before the test fails)
                worst = max(worst, compare_with_oracle(got, ref, stable, probs[name], (name, n, of)))
            except AssertionError as e:
                failed.append(str(e).split("\n")[0])
    print("  (a) n = %d: worst pose difference %.2e" % (n, worst))
    assert not failed, failed


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.STEP_N)
def test_one_step_matches_independent_reference(P, opt, n):
    wp = wf = 0.0
    for of in R.OUTLIER_FRACS:
        probs, _ = R.scene_problems(P, n, R.case_seed(n, of), of)
        for name in R.BUILDERS:
            q = R.as_one_step(probs[name])
            one = R.one_step(q)                                      # the flow problems: dense (6 + 2 n) form up to n = 257, eliminated above
            assert one["chi2_after"] < one["chi2_before"], (name, n, of)
            got = opt.pose_optimize(q)
            dp, df = np.abs(got["T"] - one["T"]).max(), np.abs(got["flow"] - one["flow"]).max()
            wp, wf = max(wp, dp), max(wf, df)
            assert dp <= 100 * R.D_STEP_POSE and df <= 100 * R.D_STEP_FLOW, (name, n, of, dp, df)
            assert got["lm_iterations"] == 1 and not got["outlier"].any() and got["n_inliers"] == n, (name, n, of)
    print("  (b) n = %d: worst difference from one_step: pose %.2e flow %.2e" % (n, wp, wf))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.EDGE_N)
def test_ground_truth_all_modes(P, oracle, opt, n):
    probs, truth = R.scene_problems(P, n, R.case_seed(n, 0.0), 0.0, noise_px=0.0, objmot_init="perturbed")
    for name in R.BUILDERS:
        pr = probs[name]
        ref, got = oracle.pose_optimize(pr), opt.pose_optimize(pr)
        true_flow = pr["flow0"] if pr["mode"] == 1 else np.zeros((n, 2))
        ep, ef = np.abs(ref["T"] - truth[name]).max(), np.abs(ref["flow"] - true_flow).max()
        gp, gf = np.abs(got["T"] - truth[name]).max(), np.abs(got["flow"] - true_flow).max()
        print("  (c) %-8s n = %4d: error against the truth: oracle %.2e / %.2e, gpu %.2e / %.2e" % (name, n, ep, ef, gp, gf))
        assert ep <= ORACLE_TRUTH_ERR[0] and ef <= ORACLE_TRUTH_ERR[1], "re-measure ORACLE_TRUTH_ERR"
        assert gp <= 100 * ORACLE_TRUTH_ERR[0] and gf <= 100 * ORACLE_TRUTH_ERR[1], (name, n, gp, gf)
        assert got["n_inliers"] == n and not got["outlier"].any()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_small_problems_do_not_depend_on_the_batch(P, opt):
    """alone a small problem runs in a 64- or 128-thread workgroup, next to a 6000-point problem in a 512-thread one: same bits"""
    small = []
    for n in (3, 5, 64, 257):
        probs, _ = R.scene_problems(P, n, R.case_seed(n, 0.05), 0.05)
        small += [probs[name] for name in R.BUILDERS]
    big = R.scene_problems(P, 6000, R.case_seed(6000, 0.05), 0.05)[0]["flow2"]
    batch = opt.pose_optimize_batch(small + [big])
    for pr, b in zip(small + [big], batch):
        assert same_bits(opt.pose_optimize(pr), b), (pr["mode"], pr["n"])
    assert all(b["lm_iterations"] > 0 for b in batch)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_launch_splitting_keeps_clusters_whole(P, opt):
    """ten 8-workgroup problems (80 workgroups: more than the 64 of one launch) interleaved with 1- and 2-workgroup ones so that the first launch ends at 63
    workgroups with an 8-workgroup cluster next: it must move to the second launch whole"""
    names = R.BUILDERS
    B = [capped(R.scene_problems(P, 4097, 4100 + i, 0.05)[0][names[i % 4]]) for i in range(10)]
    g1 = [capped(R.scene_problems(P, 64 + i, 4200 + i, 0.05)[0][names[i % 4]]) for i in range(2)]
    g2 = [capped(R.scene_problems(P, 1000 + i, 4300 + i, 0.05)[0][names[i % 4]]) for i in range(4)]
    order = [g1[0]] + B[:7] + g2[:3] + [B[7], g1[1], B[8], g2[3], B[9]]
    sizes = [min(8, max(1, (p["n"] + 511) // 512)) for p in order]
    assert sum(sizes[:11]) == 63 and sizes[11] == 8 and sum(sizes) == 90
    batch = opt.pose_optimize_batch(order)
    for pr, b in zip(order, batch):
        assert b["lm_iterations"] > 0
        assert same_bits(opt.pose_optimize(pr), b), (pr["mode"], pr["n"])


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_growth_and_reuse(vido, P):
    one = [R.scene_problems(P, 100, 5000, 0.05)[0]["flow2cam"]]
    forty = [R.scene_problems(P, 30 + 3 * i, 5001 + i, 0.05)[0][R.BUILDERS[i % 4]] for i in range(40)]      # 40 > prob_cap = 2 * 1 + 8: the exchange areas are reallocated
    clustered = [R.scene_problems(P, 2049, 5100, 0.05)[0]["flow2cam"]]
    calls = [one, forty, clustered]
    got = on_fresh_context(vido, lambda o: [o.pose_optimize_batch(c) for c in calls])
    for c, g in zip(calls, got):
        fresh = on_fresh_context(vido, lambda o: o.pose_optimize_batch(c))
        assert all(same_bits(a, b) for a, b in zip(g, fresh)), len(c)


def test_clustered_problem_fifty_times(opt, P):
    """the epoch tags of launch k must not be mistaken for those of launch k + 1: same bits every time"""
    pr = capped(R.scene_problems(P, 2049, 5200, 0.05)[0]["flow2"])
    first = opt.pose_optimize(pr)
    assert first["lm_iterations"] > 1
    for k in range(49):
        assert same_bits(opt.pose_optimize(pr), first), k


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_fewer_than_three_points_inside_a_batch(P, oracle, opt):
    real = R.scene_problems(P, 300, 6000, 0.05)[0]
    tiny = []
    for n in (0, 1, 2):
        s = P.synth_pose_scene(max(n, 1), seed=6001 + n)
        cut = {k: (v[:n] if k in ("uv_last", "depth", "Xw", "uv_cur", "flow") else v) for k, v in s.items()}
        tiny += [P.pose_problem_new(cut["Xw"], cut["uv_cur"], s["K"], s["T_init"]),
                 P.pose_problem_flow2cam(cut["uv_last"], cut["flow"], cut["depth"], s["Twl"], s["K"], s["T_init"]),
                 P.pose_problem_objmot(cut["Xw"], cut["uv_cur"], s["K"], s["T_cur"], s["T_init"])]
    order = [real["new"]] + tiny[:4] + [real["flow2cam"]] + tiny[4:] + [real["objmot"]]
    batch = opt.pose_optimize_batch(order)
    for pr, b in zip(order, batch):
        if pr["n"] >= 3:
            assert same_bits(opt.pose_optimize(pr), b)
            continue
        ref = oracle.pose_optimize(pr)
        for r in (ref, b):
            assert np.array_equal(r["T"], pr["T_init"]) and r["lm_iterations"] == 0 and r["n_inliers"] == 0 and not r["outlier"].any() and r["outlier"].shape == (pr["n"],)
        assert np.array_equal(b["flow"], ref["flow"])


@pytest.mark.parametrize("n", [40, 700])
def test_garbage_correspondences(P, oracle, opt, n):
    """every match is wrong: after round 1 of flow2cam every edge is an outlier and the pose block of H is zero"""
    s = P.synth_pose_scene(n, seed=6100 + n)
    rng = np.random.RandomState(6200 + n)
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    probs = {"new": P.pose_problem_new(s["Xw"], uv, s["K"], s["T_init"]),
             "flow2cam": P.pose_problem_flow2cam(s["uv_last"], uv - s["uv_last"], s["depth"], s["Twl"], s["K"], s["T_init"]),
             "flow2": P.pose_problem_flow2(s["uv_last"], uv - s["uv_last"], s["depth"], s["Twl"], s["K"], s["T_init"]),
             "objmot": P.pose_problem_objmot(s["Xw"], uv, s["K"], s["T_cur"], np.eye(4))}
    first_round = dict(probs["flow2cam"]); first_round["rounds"] = 1
    assert oracle.pose_optimize(first_round)["outlier"].all()
    for name, pr in probs.items():
        ref, stable, _ = R.order_stability(oracle, pr, ("garbage", name, n))
        got = opt.pose_optimize(pr)
        d = compare_with_oracle(got, ref, stable, pr, ("garbage", name, n))
        print("  (g) garbage %-8s n = %3d: %-12s inliers %d, pose difference %.2e" % (name, n, "order-stable" if stable else "NOT stable", got["n_inliers"], d))


# ---- (h) ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_inputs_leave_the_context_usable(vido, P):
    good = R.scene_problems(P, 1025, 7000, 0.05)[0]
    valid = capped(good["flow2cam"])
    expect = on_fresh_context(vido, lambda o: o.pose_optimize(valid))
    bad = {}
    for name, change in (("rounds 0", dict(rounds=0)), ("rounds 5", dict(rounds=5)), ("negative iters", dict(iters=[100, -1, 100, 100])),
                         ("iteration sum past the epoch window", dict(iters=[195, 195, 195, 195])),           # 21 * 780 + 4 + 1 = 16385 >= 2^14
                         ("mode 3", dict(mode=3)), ("null obs", dict(obs=None))):
        bad[name] = dict(good["flow2cam"]); bad[name].update(change)
    last_allowed = dict(good["flow2cam"]); last_allowed["iters"] = [195, 195, 195, 194]                        # 21 * 779 + 5 = 16364 < 2^14

    def run(o):
        for name, pr in bad.items():
            with pytest.raises(vido.VidoError):
                o.pose_optimize(pr)
            with pytest.raises(vido.VidoError):
                o.pose_optimize_batch([valid, pr])
            assert same_bits(o.pose_optimize(valid), expect), name
        full = o.pose_optimize(good["flow2cam"])
        assert same_bits(o.pose_optimize(last_allowed), full) and full["lm_iterations"] < 100       # (both stop by convergence)
    on_fresh_context(vido, run)
