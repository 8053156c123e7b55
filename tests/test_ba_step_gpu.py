"""Step-level parity of vido_ba_optimize (csrc/ba.hip) with the CPU oracle on every Schur kernel, reduced solver and Levenberg-Marquardt driver.

tests/test_ba_gpu.py compares converged solves at 1e-4: LM corrects itself, so a solver that drops a small term still converges to the same minimum and passes.  Here one
to four iterations on graphs of a few hundred landmarks (tests/refimpl/ba_cases.py) are compared with oracle.ba_optimize at

    |got - ref| <= 1e-9 * step + 100 * floor        elementwise, cam_T and pt_xyz

    step  = max |ref - initial|: what the compared iterations moved
    floor = max |ref - ref2|, ref2 = oracle.badyn_optimize with an empty object part: what two honest fp64 algorithms on the CPU differ by on this input

1e-9 * step: a backward-stable solve has relative forward error ~ cond * eps; cond(S) <= 3e5 for every case (tests/test_ba_step_cpu.py), so cond * eps ~ 3e-11, and the
factor 30 above it covers the free summation order of the device (up to 17 k atomically added terms), the larger constant of cyclic reduction and the 3x3 inverses written
differently.  A dropped term shows at 1e-6 of a step or more.  chi2_initial, chi2_final and lambda_final: 1e-9 relative; (iterations, lm_trials): equal.

Every test also reads the `[ba] path:` line of VIDO_BA_VERBOSE and compares it with the path the case is listed for (and that ba_cases.host_path derives from the problem),
so that a threshold moved in the host code fails here instead of silently running another kernel.

The rejected-trial cases (`hard_*`: ba_cases.hard_start) run the `rho <= 0` branch of both drivers: the host loop's (restore, lambda *= ni, ni *= 2) and the device-resident
driver's in k_bas_backsub; hard_local20_gauge_free at max_iters = 4 needs 7 trial slots, more than the first budget of 4, so the refill loop runs as well.

Observed on the MI355X (err = max |got - ref| over cam_T and pt_xyz; bound = 1e-9 * step + 100 * floor):
  case                     schur / solver / driver          k  (it,tr) step     floor    bound     err       err/bound
  one_camera               schur0 / small / host            1  (1, 1)  0.0304   3.8e-17  3.05e-11  2.8e-17   9.1e-07 
  one_camera               schur0 / small / host            2  (2, 2)  0.0304   1.1e-19  3.04e-11  1.1e-19   3.7e-09 
  local3                   schur0 / small6 / resident       1  (1, 1)  0.0378   2.1e-17  3.78e-11  1.4e-17   3.7e-07 
  local3                   schur0 / small6 / resident       2  (2, 2)  0.0488   1.4e-17  4.88e-11  2.1e-17   4.3e-07 
  local5                   schur0 / small6 / resident       1  (1, 1)  0.0565   6.9e-17  5.66e-11  2.8e-17   4.9e-07 
  local5                   schur0 / small6 / resident       2  (2, 2)  0.0819   4.2e-17  8.19e-11  2.1e-17   2.5e-07 
  local20_gauge_free       schur0 / small6 / resident       1  (1, 1)  0.34     7.1e-15  3.41e-10  7.1e-15   2.1e-05 
  local20_gauge_free       schur0 / small6 / resident       2  (2, 2)  0.528    3.3e-14  5.31e-10  4e-14     7.5e-05 
  local20_hook             schur0 / small6 / host           1  (1, 1)  0.0807   1.8e-15  8.08e-11  1.1e-16   1.4e-06 
  local20_hook             schur0 / small6 / host           2  (2, 2)  0.092    1.8e-15  9.22e-11  2.2e-16   2.4e-06 
  local21_dense            schur2 / dense / host            1  (1, 1)  0.091    2.1e-16  9.1e-11   1.1e-16   1.2e-06 
  local21_dense            schur2 / dense / host            2  (2, 2)  0.108    1.1e-16  1.08e-10  8.9e-16   8.2e-06 
  g23_band6                mfma / band6 / host              1  (1, 1)  0.12     1.8e-15  1.2e-10   1.8e-15   1.5e-05 
  g23_band6                mfma / band6 / host              2  (2, 2)  0.144    1.8e-15  1.44e-10  1.8e-15   1.2e-05 
  g23_20pt                 schur2 / band6 / host            1  (1, 1)  0.133    2.3e-16  1.33e-10  2.8e-16   2.1e-06 
  g23_20pt                 schur2 / band6 / host            2  (2, 2)  0.126    3.6e-15  1.26e-10  3.6e-15   2.8e-05 
  g23_20_in_window         mfma / band6 / host              1  (1, 1)  0.107    3e-16    1.07e-10  3.5e-16   3.2e-06 
  g23_20_in_window         mfma / band6 / host              2  (2, 2)  0.131    1.8e-15  1.31e-10  1.8e-15   1.4e-05 
  g60_bcr66                schur2 / bcr66 / host            1  (1, 1)  0.146    3.6e-15  1.46e-10  3.6e-15   2.4e-05 
  g60_bcr66                schur2 / bcr66 / host            2  (2, 2)  0.174    7.1e-15  1.75e-10  7.1e-15   4.1e-05 
  g80_bcr96                schur2 / bcr96 / host            1  (1, 1)  0.138    1.8e-15  1.38e-10  3.6e-15   2.6e-05 
  g80_bcr96                schur2 / bcr96 / host            2  (2, 2)  0.146    1.4e-14  1.47e-10  1.4e-14   9.6e-05 
  g60_no_bcr               schur2 / band6 / host            1  (1, 1)  0.146    3.6e-15  1.46e-10  3.6e-15   2.4e-05 
  g60_no_bcr               schur2 / band6 / host            2  (2, 2)  0.174    7.1e-15  1.75e-10  7.1e-15   4.1e-05 
  g90_band6s8              schur2 / band6s8 / host          1  (1, 1)  0.136    1.4e-14  1.38e-10  1.4e-14   0.0001  
  g90_band6s8              schur2 / band6s8 / host          2  (2, 2)  0.159    1.4e-14  1.6e-10   1.4e-14   8.9e-05 
  g130_band6s4             schur2 / band6s4 / host          1  (1, 1)  0.166    1.4e-14  1.67e-10  1.4e-14   8.5e-05 
  g130_band6s4             schur2 / band6s4 / host          2  (2, 2)  0.177    1.4e-14  1.79e-10  1.4e-14   8e-05   
  g210_band_long           schur2+long 111 / band / host    1  (1, 1)  0.175    1.4e-14  1.77e-10  1.4e-14   8e-05   
  g210_band_long           schur2+long 111 / band / host    2  (2, 2)  0.213    1.4e-14  2.14e-10  1.4e-14   6.6e-05 
  g100_revisit_10pct       schur2 / dense / host            1  (1, 1)  0.166    1.4e-14  1.67e-10  1.4e-14   8.5e-05 
  g100_revisit_10pct       schur2 / dense / host            2  (2, 2)  0.169    1.4e-14  1.7e-10   1.4e-14   8.4e-05 
  g100_revisit_half_pct    schur2 / dense / host            1  (1, 1)  0.166    1.4e-14  1.67e-10  1.4e-14   8.5e-05 
  g100_revisit_half_pct    schur2 / dense / host            2  (2, 2)  0.169    7.1e-15  1.69e-10  7.1e-15   4.2e-05 
  g40_revisit_near         mfma+long 6 / dense / host       1  (1, 1)  0.127    7.1e-15  1.28e-10  8.9e-16   7e-06   
  g40_revisit_near         mfma+long 6 / dense / host       2  (2, 2)  0.147    7.1e-15  1.48e-10  7.1e-15   4.8e-05 
  hard_local20_gauge_free  schur0 / small6 / resident       2  (2, 5)  17.4     1.2e-10  2.95e-08  1.2e-10   0.0041  
  hard_local20_gauge_free  schur0 / small6 / resident       4  (4, 7)  13.1     1.1e-10  2.4e-08   1.1e-10   0.0045  
  hard_local12             schur0 / small6 / resident       4  (4, 6)  2.5      1.5e-12  2.65e-09  1.5e-12   0.00058 
  hard_g23_band6           mfma / band6 / host              1  (1, 3)  4.22     6.3e-13  4.28e-09  6.2e-13   0.00014 
  hard_g23_band6           mfma / band6 / host              4  (4, 7)  7.04     4.5e-12  7.5e-09   5e-12     0.00066 
  hard_g60_bcr66           schur2 / bcr66 / host            1  (1, 3)  4.92     8.1e-13  5e-09     7.7e-13   0.00015 
  hard_g60_bcr66           schur2 / bcr66 / host            4  (4, 7)  7.32     5.7e-12  7.88e-09  6e-12     0.00076 
  hard_g80_bcr96           schur2 / bcr96 / host            1  (1, 3)  5.51     7.5e-12  6.25e-09  5.7e-12   0.00092 
  hard_g80_bcr96           schur2 / bcr96 / host            4  (4, 6)  6.55     1.2e-11  7.8e-09   7.8e-12   0.001   
  hard_local21_dense       schur2 / dense / host            4  (4, 6)  3.35     1.7e-12  3.52e-09  6.1e-13   0.00017 
  hard_local20_hook        schur0 / small6 / host           4  (4, 6)  3.3      1.7e-12  3.47e-09  1.7e-12   0.0005  
  dynamic hard start       schur0 / small6 / host           1  (1, 3)  5.12     8.7e-13  5.21e-09  1.1e-13   2.1e-05
  dynamic hard start       schur0 / small6 / host           2  (2, 4)  5.2      1.3e-12  5.33e-09  4.8e-13   9e-05
The GPU sits at the floor of the two CPU algorithms on every path (err ~ floor); the largest share of the bound used is 0.45 % (the resident driver after 7 trials from the
hard start, where `floor` itself is 1e-10).  The slot-budget test's three runs differ among themselves by less than 1e-14 (mild) and agree to the printed digits (hard).

The object part: a hard_start variant of test_dynamic_ba_first_step_exact was ADDED (test_dynamic_ba_steps_from_a_hard_start): the dense dynamic oracle
rejects two trials in its first iteration, (iterations, lm_trials) = (1, 3) and (2, 4), and agrees with the sparse (SuperLU) solve of the same system to 2.5e-13 of the step
(tests/test_ba_step_cpu.py).

Paths: at a few hundred landmarks only the 23- and 40-camera global graphs are dense enough for the matrix-core Schur kernel (a unit of 64 landmarks must fit its 16-camera
window); g23_20pt (20 landmarks spread over 23 cameras) therefore runs k_ba_schur<2>, and g23_20_in_window (20 consecutive landmarks of the 300) is the launch of
k_ba_schur_mfma with less than one 32-landmark pass.  In g210_band_long 111 of the 120 tracks are longer than 64 frames (k_ba_schur_long); the other 9 leave the window, which
is more than 3 %, so the wave-per-landmark kernel takes them.  Both 100-camera revisit graphs run k_ba_schur<2> and the dense solver at 400 landmarks (a revisit widens the
band past n6 / 2); g40_revisit_near (revisits 20 and 25 frames later, 600 landmarks) is the k_ba_schur_mfma + k_ba_schur_long combination.

Each test fails on a kernel that is subtly wrong.  Numeric one-line mutations of csrc/ba.hip (a factor 1 + 1e-6 on one term, or a dropped update of the damping growth),
built as variant libraries and run once each against this module and tests/test_ba_gpu.py::test_ba_matches_oracle (which passed, all seven configurations, under every one):
  * ba_schur_body: pair term WD_i W_j^T x (1 + 1e-6)         -> 22 fail: local20_gauge_free, g60_bcr66, g60_no_bcr, g90_band6s8, g130_band6s4 (both k), g80_bcr96-2, g210_band_long-2,
                                                                both revisit graphs at k = 2, hard_local20_gauge_free, hard_local12, hard_g80_bcr96-4, hard_local21_dense,
                                                                hard_local20_hook, both slot-budget tests
  * k_ba_schur_mfma: rhs flush x (1 + 1e-6)                  -> 5 fail: g23_band6 (both k), g23_20_in_window-2, g40_revisit_near (both k)
  * k_ba_schur_long: rhs term x (1 + 1e-6)                   -> 2 fail: g210_band_long (both k)
  * k_bcr_update4: D_a -= dv x (1 + 1e-6)                    -> 8 fail: g60_bcr66, g80_bcr96, hard_g60_bcr66, hard_g80_bcr96 (every k)
  * k_chol_band: trailing update x (1 + 1e-6)                -> 2 fail: g210_band_long (both k)
  * k_chol_band6: panel row term x (1 + 1e-6)                -> 10 fail: g23_band6, g23_20pt, g23_20_in_window, g60_no_bcr, hard_g23_band6 (every k)
  * k_chol_band6s: panel row term x (1 + 1e-6)               -> 4 fail: g90_band6s8, g130_band6s4 (both k)
  * k_chol_update (dense): trailing update x (1 + 1e-6)      -> 9 fail: local21_dense, the three revisit graphs (both k), hard_local21_dense
  * small6 backward sweep: rW[j] -= sum x (1 + 1e-6)         -> 16 fail: local3, local5, local20_gauge_free, local20_hook (both k), the hard local cases, both slot-budget tests,
                                                                both dynamic tests
  * k_ba_backsub: x0 x (1 + 1e-6)                            -> 40 fail: every host-driver case, both dynamic tests
  * resident back substitution: x0 x (1 + 1e-6)              -> 11 fail: every resident-driver case, both slot-budget tests
  * host loop, rejected trial: `ni *= 2` dropped             -> 10 fail: every hard_* case of the host driver, both dynamic tests (lm_trials and lambda_final differ)
  * k_bas_backsub, rejected trial: `s.ni *= 2` dropped       -> 4 fail: hard_local20_gauge_free (both k), hard_local12, the hard slot-budget test
"""
import re
import numpy as np
import pytest

from refimpl import ba_cases as B

pytestmark = pytest.mark.gpu
PATH_RE = re.compile(r"\[ba\] path: schur (\w+) schur_long (\d+) \| solver (\w+) \| driver (\w+)")


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=640, height=480, max_batch=1)
    yield c
    c.close()


def _solve(vido, ctx, cid, max_iters, monkeypatch, capfd):
    """one solve of the case with the verbose line captured -> (result, (schur, schur_long, solver, driver))"""
    from vido_slam_amd.host import ALLREDUCE_FN
    c = B.CASES[cid]; pr = B.problem(cid, max_iters)
    monkeypatch.setenv("VIDO_BA_VERBOSE", "1")
    if c["no_bcr"]:
        monkeypatch.setenv("VIDO_BA_NO_BCR", "1")
    else:
        monkeypatch.delenv("VIDO_BA_NO_BCR", raising=False)
    kw = {}
    if c["hooked"]:                       # world 1 through the sharded code path: the reduction over one rank is the identity
        hook = ALLREDUCE_FN(lambda user, ptr, count, op: 0)
        kw = dict(rank=0, world=1, shard=(0, int(pr["n_pt"])), allreduce=hook)
    seen = capfd.readouterr()
    got = vido.ba_optimize(ctx, pr, **kw)
    m = PATH_RE.findall(capfd.readouterr().err)
    print(seen.out, end="")                # (what the test printed before this solve stays in its captured output)
    assert len(m) == 1, m
    return got, (m[0][0], int(m[0][1]), m[0][2], m[0][3])


def _check(cid, max_iters, got, tag=""):
    R = B.reference(cid, max_iters); ref = R["ref"]
    bound = 1e-9 * R["step"] + 100 * R["floor"]
    e_cam = np.abs(got["cam_T"] - ref["cam_T"]).max(); e_pt = np.abs(got["pt_xyz"] - ref["pt_xyz"]).max()
    print("\n[ba step] %-24s it %d%s | (it, trials) %s ref %s | step %.3g floor %.2g bound %.3g | err cam %.3g pt %.3g = %.2g of the bound | chi2 %.2g lambda %.2g" % (
        cid, max_iters, tag, (got["iterations"], got["lm_trials"]), (ref["iterations"], ref["lm_trials"]), R["step"], R["floor"], bound, e_cam, e_pt, max(e_cam, e_pt) / bound,
        abs(got["chi2_final"] - ref["chi2_final"]) / ref["chi2_final"], abs(got["lambda_final"] - ref["lambda_final"]) / ref["lambda_final"]))
    assert (got["iterations"], got["lm_trials"]) == (ref["iterations"], ref["lm_trials"])
    assert np.all(np.abs(got["cam_T"] - ref["cam_T"]) <= bound), (e_cam, bound)
    assert np.all(np.abs(got["pt_xyz"] - ref["pt_xyz"]) <= bound), (e_pt, bound)
    for key in ("chi2_initial", "chi2_final", "lambda_final"):
        assert abs(got[key] - ref[key]) <= 1e-9 * abs(ref[key]), (key, got[key], ref[key])


@pytest.mark.parametrize("cid,max_iters", B.RUNS, ids=["%s-%d" % r for r in B.RUNS])
def test_ba_steps_match_the_oracle_on_the_listed_path(vido, oracle, ctx, monkeypatch, capfd, cid, max_iters):
    c = B.CASES[cid]
    got, (schur, n_long, solver, driver) = _solve(vido, ctx, cid, max_iters, monkeypatch, capfd)
    print("\n[ba step] %-24s path: %s (schur_long %d) / %s / %s" % (cid, schur, n_long, solver, driver))
    assert (schur, solver, driver) == (c["schur"], c["solver"], c["driver"])
    hp = B.host_path(B.problem(cid, max_iters), c["hooked"], c["no_bcr"])
    assert (schur, n_long, solver, driver) == (hp["schur"], hp["schur_long"], hp["solver"], hp["driver"])
    if c["hard"]:
        assert got["lm_trials"] > got["iterations"]              # trials were rejected, on this driver
    _check(cid, max_iters, got)


@pytest.mark.parametrize("cid", ["local5", "g23_band6"])
def test_zero_iterations_return_the_input(vido, oracle, ctx, cid):
    """max_iters = 0: the estimate comes back bit-identical, no iteration and no trial is counted, both chi2 are the input's (the oracle leaves its own chi2_final unset
    here, so the reference is oracle.ba_chi2)"""
    pr = B.problem(cid, 0)
    got = vido.ba_optimize(ctx, pr)
    assert got["iterations"] == 0 and got["lm_trials"] == 0
    assert np.array_equal(got["cam_T"], np.asarray(pr["cam_T"])) and np.array_equal(got["pt_xyz"], np.asarray(pr["pt_xyz"]))
    chi = oracle.ba_chi2(pr)
    assert got["chi2_final"] == got["chi2_initial"] and abs(got["chi2_initial"] - chi) <= 1e-12 * chi, (got["chi2_initial"], chi)


@pytest.mark.parametrize("cid,max_iters", [("local20_gauge_free", 2), ("hard_local20_gauge_free", 4)])
def test_resident_driver_does_not_depend_on_its_slot_budget(vido, oracle, monkeypatch, capfd, cid, max_iters):
    """The device-resident driver enqueues (trials of the context's previous solve + 2) trial slots, at least 4, and four more at a time when a solve needs more.  The same
    case twice on one context, then on a context that has solved nothing: the budget of a cold context (the hard start's 7 trials refill it), the budget left by the previous
    solve, and a cold one again.  Every run is within the tolerance of the oracle."""
    a = vido.Context(width=640, height=480, max_batch=1); b = vido.Context(width=640, height=480, max_batch=1)
    try:
        for n, c in enumerate((a, a, b)):
            got, path = _solve(vido, c, cid, max_iters, monkeypatch, capfd)
            assert path[3] == "resident"
            _check(cid, max_iters, got, tag=" run %d" % n)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("max_iters", sorted(B.DYN_RUNS))
def test_dynamic_ba_steps_from_a_hard_start(vido, oracle, ctx, monkeypatch, capfd, max_iters):
    """tests/test_badyn_gpu.py::test_dynamic_ba_first_step_exact's graph (7 cameras, 2 objects) from ba_cases.hard_start: the dense oracle rejects two trials in the first
    iteration, so the host loop's rejection branch runs with the object part (k_badyn_factor / k_badyn_schur / k_badyn_backsub at the larger lambdas, the dynamic
    points' trial state swapped back).  Reference: the dense un-eliminated solve; floor: its difference to the sparse (SuperLU) solve of the same system."""
    base, dyn = B.dynamic_problem(max_iters)
    R = B.dynamic_reference(max_iters); ref = R["ref"]; bound = 1e-9 * R["step"] + 100 * R["floor"]
    monkeypatch.setenv("VIDO_BA_VERBOSE", "1"); capfd.readouterr()
    got = vido.ba_optimize(ctx, base, dynamic=dyn)
    assert PATH_RE.findall(capfd.readouterr().err) == [("schur0", "0", "small6", "host")]          # 7 cameras + 9 object motions: n6 = 96, the LDS-resident system
    err = {k: float(np.abs(got[k] - ref[k]).max()) for k in B.DYN_KEYS}
    print("\n[ba step] dynamic hard start it %d | (it, trials) %s ref %s | step %.3g floor %.2g bound %.3g | err %s = %.2g of the bound" % (
        max_iters, (got["iterations"], got["lm_trials"]), (ref["iterations"], ref["lm_trials"]), R["step"], R["floor"], bound, err, max(err.values()) / bound))
    assert (got["iterations"], got["lm_trials"]) == (ref["iterations"], ref["lm_trials"]) == B.DYN_RUNS[max_iters]
    for k in B.DYN_KEYS:
        assert np.all(np.abs(got[k] - ref[k]) <= bound), (k, err[k], bound)
    for key in ("chi2_initial", "chi2_final", "lambda_final"):
        assert abs(got[key] - ref[key]) <= 1e-9 * abs(ref[key]), (key, got[key], ref[key])
