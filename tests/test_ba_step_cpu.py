"""The preconditions of tests/test_ba_step_gpu.py, checked without a GPU on the very inputs that module solves (tests/refimpl/ba_cases.py).

The GPU module compares one to four Levenberg-Marquardt iterations of vido_ba_optimize with oracle.ba_optimize at 1e-9 of the step plus 100 x `floor`, where `floor` is what
the two CPU algorithms of the oracle (point-Schur + dense LDL^T; the un-eliminated dense system) differ by.  That bound means something only if, for every case,

  * the two CPU algorithms take the same LM path and agree to 1e-10 of the step (a case that does not is replaced by another seed, not tolerated),
  * the reduced system is as well conditioned as the bound's derivation assumes (cond(S) <= 3e5: cond * eps ~ 1e-11 of a step),
  * the path restated by ba_cases.host_path is the path the case is listed for,
  * the rejected-trial cases do reject trials, with the counts they are listed with.
"""
import numpy as np
import pytest

from refimpl import ba_cases as B


@pytest.mark.parametrize("cid,max_iters", B.RUNS, ids=["%s-%d" % r for r in B.RUNS])
def test_the_two_cpu_algorithms_agree(oracle, cid, max_iters):
    R = B.reference(cid, max_iters); ref, ref2 = R["ref"], R["ref2"]; c = B.CASES[cid]
    assert (ref["iterations"], ref["lm_trials"]) == (ref2["iterations"], ref2["lm_trials"])
    assert ref["iterations"] == max_iters                                     # no case stops early: `max_iters` iterations are what is compared
    assert R["step"] > 0.01 and R["floor"] <= 1e-10 * R["step"], (R["floor"], R["step"])
    for key in ("chi2_initial", "chi2_final", "lambda_final"):
        assert abs(ref[key] - ref2[key]) <= 1e-10 * abs(ref[key]), key
    if c["hard"]:
        assert ref["lm_trials"] > ref["iterations"] and (ref["iterations"], ref["lm_trials"]) == c["trials"][max_iters]
    else:
        assert ref["lm_trials"] == ref["iterations"]                          # the mild start: every first trial is accepted


@pytest.mark.parametrize("cid", list(B.CASES))
def test_reduced_system_is_well_conditioned(oracle, cid):
    lam = oracle.ba_optimize(B.problem(cid, 1))["lambda_final"]             # the one-iteration lambda_final, at the initial estimate
    S, _, _ = oracle.ba_reduced_system(B.problem(cid, 1), lam)
    assert np.abs(S - S.T).max() <= 1e-9 * np.abs(S).max()
    w = np.linalg.eigvalsh(S)
    assert w[0] > 0 and w[-1] / w[0] <= 3e5, w[-1] / w[0]


@pytest.mark.parametrize("cid", list(B.CASES))
def test_case_takes_the_path_it_is_listed_for(cid):
    c = B.CASES[cid]; hp = B.host_path(B.problem(cid, 1), c["hooked"], c["no_bcr"])
    assert (hp["schur"], hp["solver"], hp["driver"]) == (c["schur"], c["solver"], c["driver"]), hp
    if c["schur_long"] is not None:
        assert hp["schur_long"] == c["schur_long"]


def test_path_geometry_of_the_listed_cases():
    """the numbers behind the names: n6, block half-bandwidth, BCR superblocks, which band kernel's LDS window fits"""
    def hp(cid):
        c = B.CASES[cid]
        return B.host_path(B.problem(cid, 1), c["hooked"], c["no_bcr"])
    assert hp("one_camera")["n6"] == 6 and hp("local3")["n6"] == 18 and hp("local20_gauge_free")["n6"] == 120
    d = hp("local21_dense"); assert d["n6"] == 126 and d["n6"] % 32 == 30 and d["bwc"] == -1          # ragged last block of the blocked dense Cholesky
    assert hp("g23_band6")["bwc"] == 6 and hp("g23_band6")["band6_lds"] > 0
    a = hp("g60_bcr66"); assert (a["bwc"], a["bcr_m"], a["bcr_nb"]) == (9, 66, 6)
    a = hp("g80_bcr96"); assert (a["bwc"], a["bcr_m"], a["bcr_nb"]) == (13, 96, 5)
    a = hp("g60_no_bcr"); assert a["bcr_m"] == 0 and a["band6_lds"] > 0
    a = hp("g90_band6s8"); assert a["bwc"] == 29 and a["band6_lds"] == 0 and a["band6s_nb"] == 8 and a["band6s_lds"] <= B.LDS_CAP
    a = hp("g130_band6s4"); assert a["bwc"] >= 58 and a["band6s_nb"] == 4 and a["band6s_lds"] <= B.LDS_CAP
    a = hp("g210_band_long"); assert a["bwc"] > 96 and a["band6_lds"] == 0 and a["band6s_lds"] == 0 and a["schur_long"] == 111
    a = hp("g23_20_in_window"); assert a["schur"] == "mfma" and B.problem("g23_20_in_window", 1)["n_pt"] < B.SM_L
    a = hp("g40_revisit_near"); assert a["schur"] == "mfma" and 0 < a["schur_long"] < 0.03 * 600
    assert hp("g100_revisit_10pct")["schur"] == "schur2"


def test_the_listed_landmark_and_observation_counts():
    """the generator's output for the listed seeds: a change there changes every number recorded in the GPU module"""
    want = {"local3": (40, 120), "local5": (60, 300), "local20_gauge_free": (200, 3566), "local20_hook": (200, 3513), "local21_dense": (200, 3714), "g23_band6": (300, 2100),
            "g60_bcr66": (400, 4000), "g80_bcr96": (500, 6994), "g90_band6s8": (400, 11474), "g130_band6s4": (300, 14790), "g210_band_long": (120, 11189)}
    for cid, (n_pt, n_obs) in want.items():
        pr = B.problem(cid, 1)
        assert (pr["n_pt"], len(pr["obs_cam"])) == (n_pt, n_obs), cid


def test_hard_start_and_single_camera_transforms(vido):
    pr = vido.problems.synth_ba_problem(n_cam=3, n_pt=40, kind="local", seed=2)
    h = B.hard_start(pr, seed=0)
    assert h["use_huber"] == 0 and pr["use_huber"] == 1 and np.array_equal(h["cam_T"][0], pr["cam_T"][0]) and not np.allclose(h["cam_T"][1], pr["cam_T"][1])
    rng = np.random.RandomState(0); u = np.r_[rng.normal(0, 2.0, 3), rng.normal(0, 1.5, 3)]
    E = np.linalg.inv(np.vstack([pr["cam_T"][1], [0, 0, 0, 1]])) @ np.vstack([h["cam_T"][1], [0, 0, 0, 1]])
    assert np.allclose(E, vido.problems.se3_exp(u), atol=1e-12)               # camera 1 takes the first six draws: camera 0 (the prior's) takes none
    free = dict(pr, prior_cam=-1); assert not np.allclose(B.hard_start(free, seed=0)["cam_T"][0], pr["cam_T"][0])
    s = B.single_camera(pr)
    assert s["n_cam"] == 1 and len(s["odo_i"]) == 0 and s["prior_cam"] == 0 and s["n_pt"] == len(np.unique(pr["obs_pt"][pr["obs_cam"] == 0]))
    assert np.all(s["obs_cam"] == 0) and s["obs_pt"].max() == s["n_pt"] - 1 and len(np.unique(s["obs_pt"])) == s["n_pt"]
    E = np.linalg.inv(np.vstack([pr["cam_T"][0], [0, 0, 0, 1]])) @ np.vstack([s["cam_T"][0], [0, 0, 0, 1]])
    assert np.allclose(E, vido.problems.se3_exp(np.full(6, 0.03)), atol=1e-12)


@pytest.mark.parametrize("max_iters", sorted(B.DYN_RUNS))
def test_dynamic_hard_start_rejects_trials_and_two_solvers_agree(oracle, max_iters):
    """the object part's case of the GPU module: the dense dynamic oracle rejects trials on it, and the dense and the sparse (SuperLU) solves of the un-eliminated system
    take the same LM path and agree to 1e-10 of the step"""
    R = B.dynamic_reference(max_iters); ref, ref2 = R["ref"], R["ref2"]
    assert (ref["iterations"], ref["lm_trials"]) == (ref2["iterations"], ref2["lm_trials"]) == B.DYN_RUNS[max_iters]
    assert ref["lm_trials"] > ref["iterations"]
    assert R["floor"] <= 1e-10 * R["step"], (R["floor"], R["step"])
