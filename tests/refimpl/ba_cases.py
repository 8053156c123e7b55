"""Case table of the step-level bundle-adjustment tests (tests/test_ba_step_cpu.py, tests/test_ba_step_gpu.py), plain numpy.

Three things live here so that the CPU module can check the preconditions of the GPU module on the very same inputs:

  * the problem transforms: `hard_start` (a start far enough from the minimum that Levenberg-Marquardt rejects trials), `single_camera` (a one-camera window: n6 = 6),
    `revisit` (landmarks seen again 60-70 frames after their track, as tests/test_ba_gpu.py builds them);
  * `host_path`: the path selection of vido_ba_optimize (csrc/ba.hip: the band layout, the block-cyclic-reduction / band / dense choice of the reduced solver, the
    matrix-core / wave-per-landmark choice of the Schur kernel, the device-resident driver's conditions) restated on the problem dict.  The tests compare its answer with
    the `[ba] path:` line that VIDO_BA_VERBOSE prints, so a threshold that moves in the host code fails a test instead of silently exercising another kernel;
  * `CASES` / `reference`: every case with the path it is listed for, and its two CPU references (oracle.ba_optimize: point-Schur + dense LDL^T; oracle.badyn_optimize with
    an empty object part: the un-eliminated dense system), computed once per (case, max_iters) and shared by both modules.
"""
import functools
import numpy as np

# csrc/ba.hip constants the selection depends on
BA_LDS_MAX_N6 = 120
CB_MAXBW = 959
BA_WC = 16            # camera window of the matrix-core Schur kernel
SM_L = 32             # landmarks per pass of k_ba_schur_mfma
LDS_CAP = 150 * 1024
N_CU = 256            # MI355X; the unit size below is 64 for every case here whatever the count (n_pt <= 16 k)


def se3_exp(u):
    """g2o SE3Quat::exp, (omega, upsilon) -> 4x4."""
    w = np.asarray(u[:3], np.float64); v = np.asarray(u[3:], np.float64)
    th = np.linalg.norm(w)
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-5:
        R = np.eye(3) + O + O @ O; V = R
    else:
        R = np.eye(3) + np.sin(th) / th * O + (1 - np.cos(th)) / th**2 * O @ O
        V = np.eye(3) + (1 - np.cos(th)) / th**2 * O + (th - np.sin(th)) / th**3 * O @ O
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = V @ v
    return T


def _rmul(T34, E):
    return np.ascontiguousarray((np.vstack([T34, [0, 0, 0, 1]]) @ E)[:3])


def hard_start(pr, seed=0, sigma_t=2.0, sigma_r=1.5):
    """Every camera's initial pose right-multiplied by se3_exp(r_[N(0, sigma_t, 3), N(0, sigma_r, 3)]) (camera 0 exempt when the problem has a prior), the draws in that
    order from one RandomState(seed); no robust kernel.  The first LM trial of such a start overshoots and is rejected."""
    q = dict(pr); rng = np.random.RandomState(seed); cam = np.array(pr["cam_T"], np.float64).copy()
    for i in range(pr["n_cam"]):
        if i == 0 and pr["prior_cam"] >= 0:
            continue
        cam[i] = _rmul(cam[i], se3_exp(np.r_[rng.normal(0, sigma_t, 3), rng.normal(0, sigma_r, 3)]))
    q["cam_T"] = cam; q["use_huber"] = 0
    return q


def single_camera(pr):
    """Camera 0 of a local problem and the landmarks it sees (re-indexed), no odometry edges, the prior kept, the pose perturbed by se3_exp(full(6, 0.03))."""
    sel = pr["obs_cam"] == 0
    ids = np.unique(pr["obs_pt"][sel]); remap = -np.ones(pr["n_pt"], np.int64); remap[ids] = np.arange(len(ids))
    q = dict(pr)
    q.update(n_cam=1, n_pt=len(ids), cam_T=_rmul(pr["cam_T"][0], se3_exp(np.full(6, 0.03)))[None], pt_xyz=np.ascontiguousarray(pr["pt_xyz"][ids]),
             obs_cam=np.zeros(int(sel.sum()), np.int32), obs_pt=remap[pr["obs_pt"][sel]].astype(np.int32), obs_meas=np.ascontiguousarray(pr["obs_meas"][sel]),
             odo_i=np.zeros(0, np.int32), odo_j=np.zeros(0, np.int32), odo_T=np.zeros((0, 3, 4)), prior_cam=0,
             cam_true=pr["cam_true"][:1], pt_true=pr["pt_true"][ids])
    return q


def revisit(pr, share, gaps=(60, 70), seed=5):
    """`share` of the landmarks get two extra observations from cameras `gaps` frames after their track (60 and 70: tests/test_ba_gpu.py, loop closures)."""
    rng = np.random.RandomState(seed); n_pt = pr["n_pt"]
    last = np.zeros(n_pt, np.int64); np.maximum.at(last, pr["obs_pt"], pr["obs_cam"])
    cand = np.nonzero(last + max(gaps) + 2 < pr["n_cam"])[0]; pick = rng.choice(cand, int(share * n_pt), replace=False)
    cams = np.stack([np.vstack([c, [0, 0, 0, 1]]) for c in pr["cam_true"]])
    oc, op, om = [pr["obs_cam"]], [pr["obs_pt"]], [pr["obs_meas"]]
    for l in pick:
        for gap in gaps:
            c = int(last[l]) + gap; inv = np.linalg.inv(cams[c]); Xc = inv[:3, :3] @ pr["pt_true"][l] + inv[:3, 3]
            oc.append(np.array([c], np.int32)); op.append(np.array([l], np.int32)); om.append((Xc + rng.normal(0, 0.02, 3))[None])
    q = dict(pr)
    q.update(obs_cam=np.concatenate(oc).astype(np.int32), obs_pt=np.concatenate(op).astype(np.int32), obs_meas=np.concatenate(om))
    return q


def keep_landmarks(pr, lo, hi):
    """the landmarks [lo, hi) only (re-indexed); cameras that lose all their observations stay in the graph, held by the odometry chain"""
    sel = (pr["obs_pt"] >= lo) & (pr["obs_pt"] < hi)
    q = dict(pr)
    q.update(n_pt=hi - lo, pt_xyz=np.ascontiguousarray(pr["pt_xyz"][lo:hi]), pt_true=pr["pt_true"][lo:hi], obs_cam=np.ascontiguousarray(pr["obs_cam"][sel]),
             obs_pt=(pr["obs_pt"][sel] - lo).astype(np.int32), obs_meas=np.ascontiguousarray(pr["obs_meas"][sel]))
    return q


def empty_dynamic():
    """the object part with nothing in it: oracle.badyn_optimize(pr, empty_dynamic()) is the un-eliminated dense solve of the static graph"""
    z = np.zeros(0, np.int32)
    return dict(n_H=0, n_dyn=0, n_tern=0, n_smooth=0, H_T=np.zeros((0, 3, 4)), dyn_xyz=np.zeros((0, 3)), dyn_cam=z, dyn_meas=np.zeros((0, 3)), tern_prev=z, tern_cur=z,
                tern_H=z, sm_i=z, sm_j=z, info_dyn=1.0 / 80, info_tern=1.0 / 100, info_smooth=1e3, huber_dyn=0.01, huber_tern=0.01, huber_smooth=0.01)


# ---- the host's path selection, restated ------------------------------------------------------------------
def host_path(pr, hooked=False, no_bcr=False):
    """What vido_ba_optimize launches for the static, unsharded problem `pr` (hooked: an all-reduce hook is passed; no_bcr: VIDO_BA_NO_BCR is set).  Returns n6, the block
    half-bandwidth `bwc` (-1: no band layout), the BCR superblock `bcr_m` and count `bcr_nb` (0: none), the band6 / band6s LDS bytes, and the names of the verbose line:
    `schur` (schur0 | mfma | schur2), `schur_long` (landmarks sent to k_ba_schur_long), `solver`, `driver` (resident | host)."""
    n_cam, n_pt = int(pr["n_cam"]), int(pr["n_pt"]); n6 = 6 * n_cam
    oc = np.asarray(pr["obs_cam"], np.int64); op = np.asarray(pr["obs_pt"], np.int64); no = len(oc)
    cnt = np.bincount(op, minlength=n_pt)
    cmin = np.full(n_pt, n_cam, np.int64); cmax = np.full(n_pt, -1, np.int64)
    np.minimum.at(cmin, op, oc); np.maximum.at(cmax, op, oc)
    n_odo = len(pr["odo_i"])
    lds_path = n6 <= BA_LDS_MAX_N6
    out = dict(n6=n6, bwc=-1, bcr_m=0, bcr_nb=0, band6_lds=0, band6s_lds=0, band6s_nb=0)
    bw = -1
    if not lds_path:
        bwc = int((cmax - cmin)[cnt > 0].max()) if no else 0
        if n_odo:
            bwc = max(bwc, int(np.abs(np.asarray(pr["odo_i"], np.int64) - np.asarray(pr["odo_j"], np.int64)).max()))
        if 6 * bwc + 5 <= CB_MAXBW and 6 * bwc + 6 < n6 // 2:
            bw = 6 * bwc + 5; out["bwc"] = bwc
    if bw >= 0:
        bwc = (bw - 5) // 6; wr = 6 * (bwc + 1)
        need = (wr * (wr + 1) + 3 * wr + 6 * bwc * 7 + 8) * 8
        if bwc >= 1 and need <= LDS_CAP:
            out["band6_lds"] = need
        elif 1 <= bwc <= 96:
            def need_s(nb):
                rr = 6 * (bwc + nb)
                return (rr * (6 * nb + 1) + rr + 2 * wr + 8) * 8
            out["band6s_nb"] = 8 if need_s(8) <= LDS_CAP else 4; out["band6s_lds"] = need_s(out["band6s_nb"])
        if bw + 1 <= 96 and not no_bcr:
            m = 66 if bw + 1 <= 66 else 96; nb = (n6 + m - 1) // m
            if nb >= 4:
                out["bcr_m"], out["bcr_nb"] = m, nb
    # Schur kernel
    long_ids = set(np.nonzero(cnt > 64)[0].tolist()); n_long = len(long_ids); schur = "none"
    if n_pt and lds_path:
        schur = "schur0"
    elif n_pt:
        per_cu = (n_pt + N_CU - 1) // N_CU
        chunk = max(64, min(512, ((per_cu + SM_L - 1) // SM_L) * SM_L))
        first = np.where(cnt > 0, cmin, n_cam)
        lorder = np.argsort(first, kind="stable")
        cams_of = [[] for _ in range(n_pt)]
        for c, l in zip(oc.tolist(), op.tolist()):
            cams_of[l].append(c)
        outside = []
        for q, l in enumerate(lorder.tolist()):
            if not cnt[l]:
                continue
            f0 = int(first[lorder[(q // chunk) * chunk]]); cb = 0 if f0 == n_cam else f0
            if cnt[l] > 64 or any(c < cb or c >= cb + BA_WC for c in cams_of[l]):
                outside.append(l)
        n_out_short = len(outside) - min(len(outside), n_long)
        if n_out_short * 100 > n_pt * 3:
            schur = "schur2"
        else:
            schur = "mfma"; n_long = len(long_ids | set(outside))
    out.update(schur=schur, schur_long=n_long)
    # reduced solver
    if lds_path:
        solver = "small6" if n6 >= 12 else "small"
    elif out["bcr_m"]:
        solver = "bcr%d" % out["bcr_m"]
    elif bw < 0:
        solver = "dense"
    elif out["band6_lds"]:
        solver = "band6"
    elif out["band6s_lds"]:
        solver = "band6s%d" % out["band6s_nb"]
    else:
        solver = "band"
    resident = lds_path and not hooked and n6 >= 12 and n_cam <= 64 and n_odo <= 64 and n_long == 0 and pr["max_iters"] >= 1 and n_pt > 0 and no > 0
    out.update(solver=solver, driver="resident" if resident else "host")
    return out


# ---- the cases -------------------------------------------------------------------------------------------
def _c(cid, kw, schur, solver, driver, **extra):
    d = dict(id=cid, kw=kw, schur=schur, solver=solver, driver=driver, transform=None, hooked=False, no_bcr=False, hard=False, iters=(1, 2), trials=None, schur_long=0)
    d.update(extra)
    return d


_G23 = dict(n_cam=23, n_pt=300, kind="global", track_len=7, seed=12)
_G60 = dict(n_cam=60, n_pt=400, kind="global", track_len=10, seed=11)
_G80 = dict(n_cam=80, n_pt=500, kind="global", track_len=14, seed=14)
_G100 = dict(n_cam=100, n_pt=400, kind="global", track_len=10, seed=41)
_L20 = dict(n_cam=20, n_pt=200, kind="local", seed=7)
_L21 = dict(n_cam=21, n_pt=200, kind="local", seed=3)

# D: one (and two) accepted steps on the generator's mild start.  The Schur kernel of the global cases follows from the landmark density: a unit of 64 landmarks must
# fit the 16-camera window of the matrix-core kernel, which at a few hundred landmarks only the 23-camera graph does; the sparser ones take the wave-per-landmark kernel.
MILD = [
    _c("one_camera", dict(n_cam=3, n_pt=40, kind="local", seed=2), "schur0", "small", "host", transform=("single_camera",)),
    _c("local3", dict(n_cam=3, n_pt=40, kind="local", seed=2), "schur0", "small6", "resident"),
    _c("local5", dict(n_cam=5, n_pt=60, kind="local", seed=9), "schur0", "small6", "resident"),
    _c("local20_gauge_free", dict(n_cam=20, n_pt=200, kind="local", seed=8, with_prior=False), "schur0", "small6", "resident"),
    _c("local20_hook", _L20, "schur0", "small6", "host", hooked=True),
    _c("local21_dense", _L21, "schur2", "dense", "host"),
    _c("g23_band6", _G23, "mfma", "band6", "host"),
    _c("g23_20pt", dict(_G23, n_pt=20), "schur2", "band6", "host"),
    _c("g23_20_in_window", _G23, "mfma", "band6", "host", transform=("keep", 140, 160)),
    _c("g60_bcr66", _G60, "schur2", "bcr66", "host"),
    _c("g80_bcr96", _G80, "schur2", "bcr96", "host"),
    _c("g60_no_bcr", _G60, "schur2", "band6", "host", no_bcr=True),
    _c("g90_band6s8", dict(n_cam=90, n_pt=400, kind="global", track_len=30, seed=13), "schur2", "band6s8", "host"),
    _c("g130_band6s4", dict(n_cam=130, n_pt=300, kind="global", track_len=60, seed=5), "schur2", "band6s4", "host"),
    _c("g210_band_long", dict(n_cam=210, n_pt=120, kind="global", track_len=100, seed=6, step=0.4), "schur2", "band", "host", schur_long=111),
    _c("g100_revisit_10pct", _G100, "schur2", "dense", "host", transform=("revisit", 0.10)),
    _c("g100_revisit_half_pct", _G100, "schur2", "dense", "host", transform=("revisit", 0.005)),
    _c("g40_revisit_near", dict(n_cam=40, n_pt=600, kind="global", track_len=10, seed=19), "mfma", "dense", "host", transform=("revisit", 0.01, (20, 25)), schur_long=None),
]

# E: rejected trials (hard_start, seed 0); trials[max_iters] = the oracle's (iterations, lm_trials)
HARD = [
    _c("hard_local20_gauge_free", dict(_L20, with_prior=False), "schur0", "small6", "resident", hard=True, iters=(2, 4), trials={2: (2, 5), 4: (4, 7)}),
    _c("hard_local12", dict(n_cam=12, n_pt=150, kind="local", seed=4), "schur0", "small6", "resident", hard=True, iters=(4,), trials={4: (4, 6)}),
    _c("hard_g23_band6", _G23, "mfma", "band6", "host", hard=True, iters=(1, 4), trials={1: (1, 3), 4: (4, 7)}),
    _c("hard_g60_bcr66", _G60, "schur2", "bcr66", "host", hard=True, iters=(1, 4), trials={1: (1, 3), 4: (4, 7)}),
    _c("hard_g80_bcr96", _G80, "schur2", "bcr96", "host", hard=True, iters=(1, 4), trials={1: (1, 3), 4: (4, 6)}),
    _c("hard_local21_dense", dict(_L21, seed=2), "schur2", "dense", "host", hard=True, iters=(4,), trials={4: (4, 6)}),
    _c("hard_local20_hook", dict(_L20, seed=3), "schur0", "small6", "host", hard=True, hooked=True, iters=(4,), trials={4: (4, 6)}),
]

CASES = {c["id"]: c for c in MILD + HARD}
RUNS = [(c["id"], k) for c in MILD + HARD for k in c["iters"]]


@functools.lru_cache(maxsize=None)
def _problem(cid):
    from vido_slam_amd import problems as P
    c = CASES[cid]; pr = P.synth_ba_problem(**c["kw"])
    if c["transform"]:
        pr = {"single_camera": single_camera, "revisit": revisit, "keep": keep_landmarks}[c["transform"][0]](pr, *c["transform"][1:])
    if c["hard"]:
        pr = hard_start(pr, seed=0)
    return pr


def problem(cid, max_iters):
    """a fresh dict of the case (the arrays are shared and never written: the solvers copy what they update)"""
    pr = dict(_problem(cid)); pr["max_iters"] = int(max_iters)
    return pr


@functools.lru_cache(maxsize=None)
def reference(cid, max_iters):
    """The two CPU solves of (case, max_iters), once per process.  `step` = max |ref - initial| over cam_T and pt_xyz; `floor` = max |ref - ref2| over both: what two
    honest fp64 algorithms differ by on this input."""
    from oracle import pyoracle as O
    pr = problem(cid, max_iters)
    ref = O.ba_optimize(pr); ref2 = O.badyn_optimize(pr, empty_dynamic())
    step = max(np.abs(ref["cam_T"] - np.asarray(pr["cam_T"])).max(), np.abs(ref["pt_xyz"] - np.asarray(pr["pt_xyz"])).max())
    floor = max(np.abs(ref["cam_T"] - ref2["cam_T"]).max(), np.abs(ref["pt_xyz"] - ref2["pt_xyz"]).max())
    for a in (ref["cam_T"], ref["pt_xyz"], ref2["cam_T"], ref2["pt_xyz"]):
        a.setflags(write=False)
    return dict(ref=ref, ref2=ref2, step=float(step), floor=float(floor))


# ---- the object part: tests/test_badyn_gpu.py::test_dynamic_ba_first_step_exact's graph from a hard start ------------------------------------
DYN_KEYS = ("cam_T", "pt_xyz", "H_T", "dyn_xyz")
DYN_RUNS = {1: (1, 3), 2: (2, 4)}            # max_iters -> the dense oracle's (iterations, lm_trials)


@functools.lru_cache(maxsize=None)
def _dynamic_problem():
    from vido_slam_amd import problems as P
    base = P.synth_ba_problem(n_cam=7, n_pt=50, kind="global", track_len=4, seed=12)
    dyn = P.synth_ba_dynamic(base, n_obj=2, pts_per_obj=7, seed=13)          # (its points are initialised through the mild camera estimates)
    return hard_start(base, seed=0), dyn


def dynamic_problem(max_iters):
    base, dyn = _dynamic_problem(); base = dict(base); base["max_iters"] = int(max_iters)
    return base, dict(dyn)


@functools.lru_cache(maxsize=None)
def dynamic_reference(max_iters):
    """oracle.badyn_optimize (dense un-eliminated system) and oracle.badyn_optimize_sparse (the same LM loop over SuperLU) on the hard-start dynamic graph"""
    from oracle import pyoracle as O
    base, dyn = dynamic_problem(max_iters)
    ref = O.badyn_optimize(base, dyn); ref2 = O.badyn_optimize_sparse(base, dyn)
    ini = dict(cam_T=base["cam_T"], pt_xyz=base["pt_xyz"], H_T=dyn["H_T"], dyn_xyz=dyn["dyn_xyz"])
    step = max(np.abs(ref[k] - np.asarray(ini[k])).max() for k in DYN_KEYS)
    floor = max(np.abs(ref[k] - ref2[k]).max() for k in DYN_KEYS)
    return dict(ref=ref, ref2=ref2, step=float(step), floor=float(floor))
