"""Reference of the device-resident local-BA window (csrc/bawin.hip), plain numpy (float64 / int64), no GPU.

Four parts, used by tests/test_bawin_ref_cpu.py (without a GPU) and tests/test_bawin_gpu.py:

  * `generate`: a sequence of frames from a seed.  Every feature continues exactly one feature of the previous frame (`asso[j]`, injective within a frame) or is born there
    (-1); the features of a frame stand in a random order, so `asso` is not the identity; `xyz` (f32) is distinct per feature over the whole sequence; `meas` is the chain's
    point in the camera frame plus noise.  Cameras and odometry are drawn like problems.synth_ba_problem (kind "local") draws them, the constants are ba_constants("local").
  * `tracklet_labels`: what Map::UpdateTracklets (grow_tracklets, csrc/facade.cpp) hands to vido_bawin_set_labels with every arriving frame.  A tracklet owns its features
    once it is 3 long: the quads (frame, feature, tracklet, position) of its positions 0, 1, 2 are emitted with the THIRD frame, one quad per frame from then on.
  * `walk`: the Map walk of batch_optimize (csrc/facade.cpp) over the tracklet tables the quads describe.  It follows the tracklet's own member list (position - 1 of the
    same tracklet), never `asso`, so it does not share the kernel's method.
  * `Ring`: what include/vido_c.h documents about the ring, with the chain following of k_bawin_assemble restated on `asso`, and the state after a zero-iteration solve:
    every observation row of the window holds the f32 `xyz` of the feature that started its chain.
"""
import numpy as np

from refimpl import ba_cases as BC

VIDO_OK, VIDO_E_INVALID = 0, -1
TRACK_LEN_P = ((1, 0.12), (2, 0.13), (3, 0.15), ("long", 0.60))      # chains of length 1, 2, 3 and long ones (4..24 frames)


def _iso(T):
    return np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4])


# ---- generator ------------------------------------------------------------------------------------------------
def generate(seed, sizes, n_frames, long_share=None):
    """-> dict(n_frames, n[f], asso[f] i32, meas[f] f64 [n][3], xyz[f] f32 [n][3], chain[f] i64 (the generator's own chain id per feature: bookkeeping, no method reads it),
    cam_true / cam0 [n_frames][3][4], odo_T [n_frames - 1][3][4] (frame i -> i + 1)).  sizes are cycled.  long_share: probability of a long chain (default: TRACK_LEN_P)."""
    rng = np.random.RandomState(seed)
    cams = []; T = np.eye(4)                                     # camera-to-world, a forward path with yaw jitter (synth_ba_problem)
    for i in range(n_frames):
        cams.append(T.copy())
        yaw = np.deg2rad(rng.uniform(-2, 2))
        d = np.eye(4); d[:3, :3] = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]); d[2, 3] = 1.0
        T = T @ d
    cams = np.stack(cams); inv = np.linalg.inv(cams)
    odo = np.stack([_iso(inv[i] @ cams[i + 1] @ BC.se3_exp(rng.normal(0, 1e-3, 6))) for i in range(n_frames - 1)]) if n_frames > 1 else np.zeros((0, 3, 4))
    cam0 = np.stack([_iso(cams[i] @ BC.se3_exp(rng.normal(0, 0.05, 6))) if i > 0 else _iso(cams[i]) for i in range(n_frames)])
    p = np.array([q for _, q in TRACK_LEN_P])
    if long_share is not None:
        p = np.r_[(1 - long_share) * p[:3] / p[:3].sum(), long_share]

    def born(k, f):                                              # k new chains in frame f: their world point and the number of frames they last
        kind = rng.choice(4, k, p=p); length = np.where(kind < 3, kind + 1, rng.randint(4, 25, k))
        Xc = np.stack([rng.uniform(-20, 20, k), rng.uniform(-5, 5, k), rng.uniform(5, 45, k) + length], 1)      # ahead of the camera for as long as the chain lasts
        return Xc @ cams[f][:3, :3].T + cams[f][:3, 3], length

    out = dict(n_frames=n_frames, n=[], asso=[], meas=[], xyz=[], chain=[], cam_true=np.stack([_iso(c) for c in cams]), cam0=cam0, odo_T=odo)
    pts = np.zeros((0, 3)); left = np.zeros(0, np.int64); n_chain = 0          # per chain: world point, frames left after the current one
    prev_chain = np.zeros(0, np.int64)
    for f in range(n_frames):
        n = int(sizes[f % len(sizes)])
        cont = np.nonzero(left[prev_chain] > 0)[0] if len(prev_chain) else np.zeros(0, np.int64)      # features of frame f - 1 whose chain goes on
        if len(cont) > n:
            cont = np.sort(rng.choice(cont, n, replace=False))                                     # no room: those chains end early
        k = n - len(cont)
        P, L = born(k, f)
        pts = np.concatenate([pts, P]); left = np.concatenate([left, L])
        chain = np.concatenate([prev_chain[cont], n_chain + np.arange(k)]).astype(np.int64); n_chain += k
        asso = np.concatenate([cont, -np.ones(k, np.int64)])
        order = rng.permutation(n)
        chain, asso = chain[order], asso[order].astype(np.int32)
        left[chain] -= 1
        Xc = pts[chain] @ inv[f][:3, :3].T + inv[f][:3, 3]
        meas = Xc + rng.normal(0, 1, (n, 3)) * (0.02 * np.abs(Xc[:, 2:3]))
        xyz = (pts[chain] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
        out["n"].append(n); out["asso"].append(asso); out["meas"].append(np.ascontiguousarray(meas)); out["xyz"].append(xyz); out["chain"].append(chain)
        prev_chain = chain
    allx = np.concatenate(out["xyz"]) if n_frames else np.zeros((0, 3), np.float32)
    assert len(np.unique(allx, axis=0)) == len(allx), "an xyz row repeats: take another seed"      # a row tells which feature it came from
    assert not np.any(allx[:, 0] == allx[:, 1]) and not np.any(allx[:, 0] == allx[:, 2]) and not np.any(allx[:, 1] == allx[:, 2])      # ... and which component
    return out


# ---- tracklet labels ------------------------------------------------------------------------------------------
def tracklet_labels(asso_rows):
    """asso_rows[f][j] (f >= 1): the feature of frame f - 1 that feature j of frame f continues, or -1.  -> (labels, tracklets): labels[f] = int64 [k][4] quads arriving
    with frame f, in emission order; tracklets = list of member lists [(frame, feature), ...].
    grow_tracklets: an associated feature joins the tracklet of its predecessor when that one was associated itself, else the two found a new tracklet (ids in feature
    order).  A tracklet that reaches 3 members takes ownership of all three, a longer one of its newest member; a feature stays with the highest-numbered owner."""
    labels = [np.zeros((0, 4), np.int64)]; tracklets = []; pre = np.zeros(0, np.int64); owner = {}
    for f in range(1, len(asso_rows)):
        a = np.asarray(asso_rows[f], np.int64); cur = -np.ones(len(a), np.int64); quads = []

        def own(t, k):
            e = tracklets[t][k]
            if owner.get(e, -1) <= t:
                owner[e] = t; quads.append((e[0], e[1], t, k))
        for j in np.nonzero(a != -1)[0].tolist():
            m = int(a[j])
            if f - 1 > 0 and m < len(pre) and pre[m] != -1:
                t = int(pre[m]); tracklets[t].append((f, j))
            else:
                t = len(tracklets); tracklets.append([(f - 1, m), (f, j)])
            cur[j] = t
            ln = len(tracklets[t])
            if ln == 3:
                own(t, 0); own(t, 1); own(t, 2)
            elif ln > 3:
                own(t, ln - 1)
        pre = cur
        labels.append(np.array(quads, np.int64).reshape(-1, 4))
    return labels, tracklets


# ---- the Map walk ---------------------------------------------------------------------------------------------
class Tables:
    """The Map's tracklet tables as the quads of the frames [0, N) describe them: trk / pos per (frame, feature) and the member list member[t][position]."""

    def __init__(self, n_per_frame):
        self.off = np.concatenate([[0], np.cumsum(n_per_frame)]).astype(np.int64)
        self.trk = -np.ones(self.off[-1], np.int64); self.pos = -np.ones(self.off[-1], np.int64)
        self.mem = -np.ones((0, 0), np.int64)                    # member[t][position] = flat feature index, -1: none
        self.n_applied = 0

    def apply(self, quads):
        q = np.asarray(quads, np.int64).reshape(-1, 4)
        if not len(q):
            return
        flat = self.off[q[:, 0]] + q[:, 1]
        self.trk[flat] = q[:, 2]; self.pos[flat] = q[:, 3]
        nt, npos = max(self.mem.shape[0], int(q[:, 2].max()) + 1), max(self.mem.shape[1], int(q[:, 3].max()) + 1)
        if (nt, npos) != self.mem.shape:
            m = -np.ones((nt if nt == self.mem.shape[0] else max(nt, 2 * self.mem.shape[0]), npos), np.int64); m[:self.mem.shape[0], :self.mem.shape[1]] = self.mem; self.mem = m
        self.mem[q[:, 2], q[:, 3]] = flat


def walk_ids(tables, n_per_frame, start, N):
    """-> (pid per frame of [start, N): int64 [n_f], landmark id or -1; owners: flat feature index that started each landmark).  Observations in (frame, feature) order,
    landmark ids in order of first appearance, a chain whose tracklet starts before `start` dropped whole."""
    off = tables.off; mak = -np.ones(off[-1], np.int64); owners = []; n_pt = 0
    for i in range(start, N):
        sl = slice(off[i], off[i + 1]); t = tables.trk[sl]; p = tables.pos[sl]
        lab = t != -1; new = lab & (p == 0); cont = lab & (p > 0)
        pid = -np.ones(n_per_frame[i], np.int64)
        pid[new] = n_pt + np.arange(int(new.sum())); owners.append(off[i] + np.nonzero(new)[0]); n_pt += int(new.sum())
        pf = tables.mem[t[cont], p[cont] - 1]                   # the tracklet's previous member
        ok = pf >= off[start]                                   # (flat indices grow with the frame: a member before `start` lies below its offset; -1 = unknown member)
        pm = -np.ones(len(pf), np.int64); pm[ok] = mak[pf[ok]]
        pid[cont] = pm
        mak[sl] = pid
    return [mak[off[i]:off[i + 1]] for i in range(start, N)], (np.concatenate(owners) if owners else np.zeros(0, np.int64))


def problem_from_ids(seq, start, N, pids, owners_xyz, prior_cam, max_iters, cam_T=None):
    """the flat problem dict of oracle.ba_optimize / oracle.ba_chi2 / host.ba_optimize for the window [start, N) with the given per-frame landmark ids"""
    from vido_slam_amd import problems as P
    oc, op, om = [], [], []
    for c, f in enumerate(range(start, N)):
        j = np.nonzero(pids[c] >= 0)[0]
        oc.append(np.full(len(j), c, np.int32)); op.append(pids[c][j].astype(np.int32)); om.append(np.asarray(seq["meas"][f], np.float64).reshape(-1, 3)[j])
    nc = N - start
    cam = np.array(seq["cam0"][start:N] if cam_T is None else cam_T, np.float64).reshape(nc, 3, 4)
    d = dict(n_cam=nc, n_pt=len(owners_xyz), cam_T=cam, pt_xyz=np.asarray(owners_xyz, np.float64).reshape(-1, 3),
             obs_cam=np.concatenate(oc) if oc else np.zeros(0, np.int32), obs_pt=np.concatenate(op) if op else np.zeros(0, np.int32),
             obs_meas=np.concatenate(om) if om else np.zeros((0, 3)), odo_i=np.arange(nc - 1, dtype=np.int32), odo_j=np.arange(1, nc, dtype=np.int32),
             odo_T=np.ascontiguousarray(seq["odo_T"][start:N - 1]).reshape(-1, 3, 4), prior_cam=int(prior_cam), prior_T=cam[0].copy())
    d.update(P.ba_constants("local")); d["max_iters"] = int(max_iters)
    return d


def walk(seq, labels, start, N, xyz=None, prior_cam=-1, max_iters=0, cam_T=None, upto=None):
    """The walk of batch_optimize over the tables that the quads labels[0 .. upto - 1] describe (upto: the number of frames that have arrived, default N).  xyz: the per-frame world points to take the landmarks from (default: the
    pushed ones).  -> (problem dict, per-frame landmark ids of the frames [start, N))"""
    T = Tables(seq["n"]); xyz = seq["xyz"] if xyz is None else xyz
    for f in range(N if upto is None else upto):
        T.apply(labels[f])
    pids, owners = walk_ids(T, seq["n"], start, N)
    allx = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in xyz])
    return problem_from_ids(seq, start, N, pids, allx[owners].astype(np.float64), prior_cam, max_iters, cam_T), pids


# ---- the ring -------------------------------------------------------------------------------------------------
class Ring:
    """cap_f slots keyed by frame % cap_f.  push_frame resets the slot's labels; quads of a negative frame, of a frame that is not in the ring or of a feature >= n are
    ignored, the others apply in the order given (the last one of a (frame, feature) pair holds)."""

    def __init__(self, cap_f, cap_n):
        self.cap_f, self.cap_n = cap_f, cap_n
        self.frame_of = [-1] * cap_f; self.n = [0] * cap_f
        self.meas = [np.zeros((0, 3))] * cap_f; self.xyz = [np.zeros((0, 3), np.float32)] * cap_f; self.asso = [np.zeros(0, np.int64)] * cap_f
        self.trk = [np.zeros(0, np.int64)] * cap_f; self.pos = [np.zeros(0, np.int64)] * cap_f

    def push_frame(self, frame, meas, xyz, asso=None):
        s = frame % self.cap_f; n = len(meas); assert 0 <= n <= self.cap_n and frame >= 0
        self.frame_of[s] = frame; self.n[s] = n
        self.meas[s] = np.array(meas, np.float64).reshape(-1, 3); self.xyz[s] = np.array(xyz, np.float32).reshape(-1, 3)
        self.asso[s] = -np.ones(n, np.int64) if asso is None else np.array(asso, np.int64)
        self.trk[s] = -np.ones(n, np.int64); self.pos[s] = np.zeros(n, np.int64)

    def set_labels(self, quads):
        q = np.asarray(quads, np.int64).reshape(-1, 4)
        for s in range(self.cap_f):
            fr = self.frame_of[s]
            if fr < 0:
                continue
            sel = q[(q[:, 0] == fr) & (q[:, 1] >= 0) & (q[:, 1] < self.n[s])]
            self.trk[s][sel[:, 1]] = sel[:, 2]; self.pos[s][sel[:, 1]] = sel[:, 3]       # (numpy assigns repeated indices in order: the last one holds)

    def has(self, frame):
        return frame >= 0 and self.frame_of[frame % self.cap_f] == frame

    def assemble(self, start, N):
        """k_bawin_assemble restated: -> (status, per-frame landmark ids, owners [(slot, feature)] per landmark).  A feature has a landmark when it is labelled and at
        position 0 (a new one, ids in (frame, feature) order), or labelled at a position > 0 in a frame after `start` with `asso` inside the previous frame's count and
        that feature has one.  Two features of one frame on one landmark: VIDO_E_INVALID."""
        assert all(self.has(f) for f in range(start, N))
        n_pt = 0; pids = []; owners = []; status = VIDO_OK; prev = None
        for f in range(start, N):
            s = f % self.cap_f; n = self.n[s]; lab = self.trk[s] != -1; ps = self.pos[s]; a = self.asso[s]
            new = lab & (ps == 0)
            pm = -np.ones(n, np.int64)
            if f > start:
                ok = lab & (ps > 0) & (a >= 0) & (a < len(prev))
                pm[ok] = prev[a[ok]]
            pid = np.where(new, n_pt + np.cumsum(new) - 1, pm)
            owners += [(s, int(j)) for j in np.nonzero(new)[0]]; n_pt += int(new.sum())
            got = pid[pid >= 0]
            if len(np.unique(got)) != len(got):
                status = VIDO_E_INVALID
            pids.append(pid); prev = pid
        return status, pids, owners

    def solve0(self, start, N):
        """a solve with max_iters = 0: -> (status, n_obs, n_pt); on VIDO_OK every observation row takes the f32 xyz of the feature that started its chain"""
        status, pids, owners = self.assemble(start, N)
        n_obs = int(sum((p >= 0).sum() for p in pids))
        if status != VIDO_OK:
            return status, n_obs, len(owners)
        first = np.array([self.xyz[s][j] for s, j in owners], np.float32).reshape(-1, 3)
        for c, f in enumerate(range(start, N)):
            s = f % self.cap_f; j = np.nonzero(pids[c] >= 0)[0]
            self.xyz[s][j] = first[pids[c][j]]
        return status, n_obs, len(owners)

    def read_points(self, frame):
        assert self.has(frame)
        return self.xyz[frame % self.cap_f].copy()


# ---- the scenarios of part A ----------------------------------------------------------------------------------
SCENARIOS = {
    #            cap_f, cap_n, window, sizes (cycled), frames pushed, seed
    "tiny":       dict(cap_f=4, cap_n=6, win=3, sizes=(2, 4, 6, 6, 0, 3, 5, 6, 1, 6), frames=10, seed=14),
    "ipt_edges":  dict(cap_f=5, cap_n=2100, win=4, sizes=(1023, 1024, 1025, 2047, 2048, 2049, 1, 0, 2100), frames=12, seed=5),
    "production": dict(cap_f=24, cap_n=8192, win=20, sizes=(8192, 8191, 5000, 1, 8192, 8192, 8192, 7000, 8192, 4097, 8192, 8192, 6000), frames=26, seed=7),
    "one_camera": dict(cap_f=4, cap_n=300, win=1, sizes=(200,), frames=4, seed=9, after=((0, 1), (1, 2), (2, 3), (3, 4))),
}
# one_camera: the newest frame of a stream never holds position 0 of a labelled tracklet (a tracklet is labelled with its third frame), so the single-camera windows at the
# head are empty graphs; `after` = windows solved once more after the last push, where the frames 0 and 1 do start labelled tracklets (a one-camera graph WITH landmarks)
_cache = {}


def scenario(sid):
    """-> (parameters, sequence, labels, tracklets, deliveries); deliveries[f] = the quads handed over after frame f was pushed: the frame's own, followed by a second
    copy of the quads that arrived cap_f - 1 frames earlier (their frames are older than f, and the first two positions of a tracklet that became 3 long then have left
    the ring by now: the ring must ignore those and the repeated ones change nothing).  Computed once; nothing in it is written afterwards."""
    if sid not in _cache:
        sc = SCENARIOS[sid]; seq = generate(sc["seed"], sc["sizes"], sc["frames"])
        labels, tracklets = tracklet_labels(seq["asso"])
        k = sc["cap_f"] - 1
        deliveries = [np.concatenate([labels[f], labels[f - k]]) if f - k >= 0 else labels[f] for f in range(sc["frames"])]
        for a in seq["asso"] + seq["meas"] + seq["xyz"] + labels + deliveries:
            a.setflags(write=False)
        _cache[sid] = (sc, seq, labels, tracklets, deliveries)
    return _cache[sid]


def windows(sc):
    """-> [(frames pushed so far, start, N)]: the window at the head after every push, then the scenario's `after` windows"""
    return [(N, max(0, N - sc["win"]), N) for N in range(1, sc["frames"] + 1)] + [(sc["frames"], a, b) for a, b in sc.get("after", ())]


# ---- the solve-parity cases of part C -------------------------------------------------------------------------
# one fresh ring per case: `frames` frames of `n` features pushed, the window [start, N) solved, then frame N pushed and [start + 1, N + 1) solved.  Chains are mostly long
# (long_share 0.9), so that a window of 20 cameras is as well conditioned as the local graphs of tests/refimpl/ba_cases.py.  The frames before `start` hold a tenth of the
# features: their chains run into the window and are dropped there, and nearly all of the window's chains are born in its first frame.
PARITY = {
    "w5":        dict(seed=11, n=60, frames=8, cap_f=8, start=2, N=7, prior=0, hard=False),
    "w20_prior": dict(seed=12, n=110, frames=23, cap_f=24, start=2, N=22, prior=0, hard=False),
    "w20_free":  dict(seed=12, n=110, frames=23, cap_f=24, start=2, N=22, prior=-1, hard=False),
    "w20_hard":  dict(seed=13, n=110, frames=23, cap_f=24, start=2, N=22, prior=-1, hard=True),
}
PARITY_RUNS = [(cid, k) for cid in PARITY for k in ((2, 4) if PARITY[cid]["hard"] else (1, 2))]      # (the hard start rejects its first trials in the second iteration)


def parity_case(cid):
    key = ("parity", cid)
    if key not in _cache:
        pc = PARITY[cid]; seq = generate(pc["seed"], (pc["n"] // 10,) * pc["start"] + (pc["n"],) * (pc["frames"] - pc["start"]), pc["frames"], long_share=0.9)
        labels, _ = tracklet_labels(seq["asso"])
        for a in seq["asso"] + seq["meas"] + seq["xyz"] + labels:
            a.setflags(write=False)
        _cache[key] = (pc, seq, labels)
    return _cache[key]


def parity_problem(cid, max_iters, second=False, xyz=None):
    """-> (problem dict, per-frame landmark ids, (start, N)) of the case's first or second window; xyz: the ring's state to take the landmarks from"""
    pc, seq, labels = parity_case(cid); start, N = pc["start"] + int(second), pc["N"] + int(second)
    pr, pids = walk(seq, labels, start, N, xyz=xyz, prior_cam=pc["prior"], max_iters=max_iters)
    if pc["hard"]:
        pr = BC.hard_start(pr, seed=0)
    return pr, pids, (start, N)


def references(pr):
    """the two CPU solves of `pr` (oracle.ba_optimize; oracle.badyn_optimize with an empty object part), `step` and `floor` as tests/refimpl/ba_cases.reference has them"""
    from oracle import pyoracle as O
    ref = O.ba_optimize(pr); ref2 = O.badyn_optimize(pr, BC.empty_dynamic())
    step = max(np.abs(ref["cam_T"] - np.asarray(pr["cam_T"])).max(), np.abs(ref["pt_xyz"] - np.asarray(pr["pt_xyz"])).max())
    floor = max(np.abs(ref["cam_T"] - ref2["cam_T"]).max(), np.abs(ref["pt_xyz"] - ref2["pt_xyz"]).max())
    return dict(ref=ref, ref2=ref2, step=float(step), floor=float(floor))


def state_after(xyz, pids, start, pt):
    """the ring's xyz rows after a solve wrote the landmarks `pt` (f64 [n_pt][3]) back: every observation row = f32(landmark), every other row unchanged"""
    out = [np.array(x, np.float32) for x in xyz]
    for c, pid in enumerate(pids):
        j = np.nonzero(pid >= 0)[0]
        out[start + c][j] = np.asarray(pt, np.float64)[pid[j]].astype(np.float32)
    return out
