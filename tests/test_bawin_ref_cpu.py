"""The reference of the device-resident local-BA window (tests/refimpl/bawin_np.py) checked without a GPU, on the very inputs tests/test_bawin_gpu.py runs.

  * the Map walk on a hand-written 4-frame example, the answer written out by hand;
  * the walk (which follows the tracklet tables) against the ring model (which follows `asso`, like k_bawin_assemble) on every window of every scenario: two methods, one
    answer, no tolerance;
  * the conditions every scenario has to meet to reach the edge it is listed for (a seed that does not meet them is replaced, not tolerated);
  * the preconditions of the solve-parity cases, as tests/test_ba_step_cpu.py states them for the cases of tests/test_ba_step_gpu.py.
"""
import numpy as np
import pytest

from refimpl import bawin_np as W


def _asso_ids(seq, labels, start, N, upto):
    """Independent of both the walk and the ring model: landmark ids by following `asso` feature by feature.  A feature is labelled when its chain is at least 3 long among
    the frames that have arrived; its chain's landmark exists when the chain's first feature lies in [start, N)."""
    n = seq["n"]; first = [[(f, j) for j in range(n[f])] for f in range(upto)]
    for f in range(1, upto):
        for j in range(n[f]):
            a = int(seq["asso"][f][j])
            if a != -1:
                first[f][j] = first[f - 1][a]
    total = {}
    for f in range(upto):
        for j in range(n[f]):
            total[first[f][j]] = total.get(first[f][j], 0) + 1
    ids = {}; out = []
    for f in range(start, N):
        row = -np.ones(n[f], np.int64)
        for j in range(n[f]):
            h = first[f][j]
            if total[h] >= 3 and h[0] >= start:
                row[j] = ids.setdefault(h, len(ids))
        out.append(row)
    return out


def test_walk_on_a_hand_written_example():
    """4 frames.  Chains (frame, feature):  A (0,0) (1,1) (2,0) (3,2)    B (0,1) (1,0)            C (1,2) (2,2) (3,0)    D (2,1) (3,1)    E (0,2) alone
    Tracklets in creation order: 0 = B (features in index order of frame 1: feature 0 first), 1 = A, 2 = C, 3 = D.  A is labelled with frame 2 (positions 0, 1, 2) and
    again with frame 3 (position 3); C with frame 3 (positions 0, 1, 2); B and D stay 2 long and are never labelled."""
    asso = [np.array([-1, -1, -1]), np.array([1, 0, -1]), np.array([1, -1, 2]), np.array([2, 1, 0])]
    labels, tracklets = W.tracklet_labels(asso)
    assert tracklets == [[(0, 1), (1, 0)], [(0, 0), (1, 1), (2, 0), (3, 2)], [(1, 2), (2, 2), (3, 0)], [(2, 1), (3, 1)]]
    assert [q.tolist() for q in labels] == [[], [], [[0, 0, 1, 0], [1, 1, 1, 1], [2, 0, 1, 2]], [[1, 2, 2, 0], [2, 2, 2, 1], [3, 0, 2, 2], [3, 2, 1, 3]]]
    rng = np.random.RandomState(0)
    seq = dict(n=[3, 3, 3, 3], asso=asso, meas=[rng.normal(size=(3, 3)) for _ in range(4)], xyz=[(100 * f + rng.normal(size=(3, 3))).astype(np.float32) for f in range(4)],
               cam0=np.tile(np.eye(4)[:3], (4, 1, 1)), odo_T=np.tile(np.eye(4)[:3], (3, 1, 1)))
    # the whole sequence: A is landmark 0 (first seen at (0,0)), C landmark 1 (first seen at (1,2)); observations in (frame, feature) order
    pr, pids = W.walk(seq, labels, 0, 4)
    assert [p.tolist() for p in pids] == [[0, -1, -1], [-1, 0, 1], [0, -1, 1], [1, -1, 0]]
    assert pr["obs_cam"].tolist() == [0, 1, 1, 2, 2, 3, 3] and pr["obs_pt"].tolist() == [0, 0, 1, 0, 1, 1, 0] and pr["n_pt"] == 2
    assert np.array_equal(pr["pt_xyz"], np.stack([seq["xyz"][0][0], seq["xyz"][1][2]]).astype(np.float64))
    assert np.array_equal(pr["obs_meas"], np.stack([seq["meas"][0][0], seq["meas"][1][1], seq["meas"][1][2], seq["meas"][2][0], seq["meas"][2][2], seq["meas"][3][0], seq["meas"][3][2]]))
    assert pr["odo_i"].tolist() == [0, 1, 2] and pr["odo_j"].tolist() == [1, 2, 3]
    # the window [1, 4): A began in frame 0 and is dropped whole, C is landmark 0
    pr, pids = W.walk(seq, labels, 1, 4)
    assert [p.tolist() for p in pids] == [[-1, -1, 0], [-1, -1, 0], [0, -1, -1]]
    assert pr["obs_cam"].tolist() == [0, 1, 2] and pr["obs_pt"].tolist() == [0, 0, 0] and pr["n_cam"] == 3 and pr["odo_i"].tolist() == [0, 1]
    # before frame 3 arrives C is not labelled: the window [1, 3) is empty
    pr, pids = W.walk(seq, labels, 1, 3)
    assert pr["n_pt"] == 0 and len(pr["obs_cam"]) == 0
    # the ring model gives the same ids from `asso`, and after a zero-iteration solve every observation row holds its chain's first point
    ring = W.Ring(4, 3)
    for f in range(4):
        ring.push_frame(f, seq["meas"][f], seq["xyz"][f], asso[f] if f else None); ring.set_labels(labels[f])
    assert ring.solve0(0, 4) == (W.VIDO_OK, 7, 2)
    a, c = seq["xyz"][0][0], seq["xyz"][1][2]
    assert np.array_equal(ring.read_points(1), np.stack([seq["xyz"][1][0], a, c])) and np.array_equal(ring.read_points(3), np.stack([c, seq["xyz"][3][1], a]))
    assert np.array_equal(ring.read_points(0), seq["xyz"][0])


@pytest.mark.parametrize("sid", list(W.SCENARIOS))
def test_walk_ring_model_and_asso_following_agree(sid):
    sc, seq, labels, tracklets, deliveries = W.scenario(sid)
    ring = W.Ring(sc["cap_f"], sc["cap_n"]); pushed = 0
    for upto, start, N in W.windows(sc):
        while pushed < upto:
            ring.push_frame(pushed, seq["meas"][pushed], seq["xyz"][pushed], seq["asso"][pushed] if pushed else None); ring.set_labels(deliveries[pushed]); pushed += 1
        pr, pids = W.walk(seq, labels, start, N, upto=upto)
        status, rp, owners = ring.assemble(start, N)
        assert status == W.VIDO_OK and len(owners) == pr["n_pt"]
        for a, b in zip(pids, rp):
            assert np.array_equal(a, b), (sid, start, N)
        if sid in ("tiny", "one_camera") or N in (3, sc["frames"]):          # (the per-feature Python loops: every window of the small scenarios, two of the large ones)
            for a, b in zip(pids, _asso_ids(seq, labels, start, N, upto)):
                assert np.array_equal(a, b), (sid, start, N)
        # landmark ids appear in order of first appearance, in (frame, feature) order
        seen = np.concatenate([p[p >= 0] for p in pids]) if pids else np.zeros(0, np.int64)
        firsts = seen[np.sort(np.unique(seen, return_index=True)[1])]
        assert np.array_equal(firsts, np.arange(pr["n_pt"]))


@pytest.mark.parametrize("sid", list(W.SCENARIOS))
def test_scenario_reaches_the_edges_it_is_listed_for(sid):
    sc, seq, labels, tracklets, deliveries = W.scenario(sid)
    assert seq["n"] == [sc["sizes"][f % len(sc["sizes"])] for f in range(sc["frames"])] and max(seq["n"]) <= sc["cap_n"]
    want = {"tiny": [2, 4, 6, 6, 0, 3, 5, 6, 1, 6], "ipt_edges": [1023, 1024, 1025, 2047, 2048, 2049, 1, 0, 2100, 1023, 1024, 1025], "one_camera": [200] * 4}
    if sid in want:
        assert seq["n"] == want[sid]
    else:
        assert seq["n"][:5] == [8192, 8191, 5000, 1, 8192] and len(seq["n"]) == 26 and sc["cap_f"] == 24 and sc["win"] == 20
    assert sc["frames"] > sc["cap_f"] or sid == "one_camera"                                       # the ring wraps
    if sid == "tiny":
        assert sc["frames"] >= 2 * sc["cap_f"] + 2 and 0 in seq["n"][1:-1] and set(range(7)) == set(seq["n"])
    for f in range(1, sc["frames"]):                                                              # asso: injective, inside the previous frame, not the identity overall
        a = seq["asso"][f]; a = a[a >= 0]
        assert len(np.unique(a)) == len(a) and (len(a) == 0 or a.max() < seq["n"][f - 1])
    assert any(np.any(seq["asso"][f][seq["asso"][f] >= 0] != np.nonzero(seq["asso"][f] >= 0)[0]) for f in range(1, sc["frames"]))
    lens = np.bincount([len(t) for t in tracklets], minlength=5)
    assert lens[2] >= 1 and lens[3] >= 1 and lens[4:].sum() >= 1                                   # tracklets of length exactly 2 (never labelled), 3, and longer
    labelled = {(int(q[0]), int(q[1])) for L in labels for q in L}
    assert not any(e in labelled for t in tracklets if len(t) == 2 for e in t)
    assert any(np.any(d[:, 0] < f) for f, d in enumerate(deliveries) if len(d))                    # a quad for a frame older than the one it arrives with
    assert any(np.any(d[:, 0] <= f - sc["cap_f"]) for f, d in enumerate(deliveries) if len(d)) or sid == "one_camera"      # ... for a frame that has left the ring
    dropped = with_graph = mixed = 0
    for upto, start, N in W.windows(sc):
        T = W.Tables(seq["n"])
        for f in range(upto):
            T.apply(labels[f])
        pids, owners = W.walk_ids(T, seq["n"], start, N)
        with_graph += len(owners) > 0
        for c, f in enumerate(range(start, N)):
            sl = slice(T.off[f], T.off[f + 1]); lab = T.trk[sl] != -1
            dropped += int((lab & (pids[c] < 0)).sum())                                             # labelled, but its chain began before `start`
            ipt = (seq["n"][f] + 1023) >> 10
            if ipt >= 2:                                                                          # a thread of k_bawin_assemble takes ipt consecutive features
                new = (lab & (T.pos[sl] == 0)).astype(np.int64); cont = ((pids[c] >= 0) & (T.pos[sl] > 0)).astype(np.int64)
                pad = (-len(new)) % ipt
                a = np.r_[new, np.zeros(pad, np.int64)].reshape(-1, ipt).sum(1); b = np.r_[cont, np.zeros(pad, np.int64)].reshape(-1, ipt).sum(1)
                mixed += int(((a > 0) & (b > 0)).sum())
    assert dropped >= 1 and with_graph >= 2
    if sid in ("ipt_edges", "production"):
        assert mixed >= 1                                                                         # one thread's range holds a chain start and a continuation
    if sid == "one_camera":
        assert all(N - start == 1 for _, start, N in W.windows(sc))


@pytest.mark.parametrize("cid,max_iters", W.PARITY_RUNS, ids=["%s-%d" % r for r in W.PARITY_RUNS])
def test_parity_cases_meet_the_preconditions_of_the_bound(oracle, cid, max_iters):
    """Both windows of the case.  The second window's landmarks come from the state the first solve leaves in the ring; here that state is built from the CPU reference
    (the GPU module builds it from what it reads back, and asserts the same conditions on it before it compares)."""
    pc, seq, labels = W.parity_case(cid)
    xyz = None
    for second in (False, True):
        pr, pids, (start, N) = W.parity_problem(cid, max_iters, second=second, xyz=xyz)
        assert pr["n_cam"] == N - start == (5 if cid == "w5" else 20) and 6 * pr["n_cam"] <= 120 and pr["prior_cam"] == pc["prior"]
        if not second:
            assert pr["n_pt"] >= (50 if cid == "w5" else 180) and len(pr["obs_cam"]) >= 3 * pr["n_pt"]
            T = W.Tables(seq["n"])
            for f in range(N):
                T.apply(labels[f])
            assert any(np.any((T.trk[T.off[start + c]:T.off[start + c + 1]] != -1) & (p < 0)) for c, p in enumerate(pids))          # a chain from before `start` is dropped
        R = W.references(pr); ref, ref2 = R["ref"], R["ref2"]
        assert (ref["iterations"], ref["lm_trials"]) == (ref2["iterations"], ref2["lm_trials"])
        assert ref["iterations"] == max_iters
        assert R["step"] > 0.01 and R["floor"] <= 1e-10 * R["step"], (R["floor"], R["step"])
        for key in ("chi2_initial", "chi2_final", "lambda_final"):
            assert abs(ref[key] - ref2[key]) <= 1e-10 * abs(ref[key]), key
        if pc["hard"] and not second:
            assert ref["lm_trials"] > ref["iterations"]                                          # the resident driver has trials to reject
        elif not pc["hard"]:
            assert ref["lm_trials"] == ref["iterations"]
        lam = oracle.ba_optimize(dict(pr, max_iters=1))["lambda_final"]
        S, _, _ = oracle.ba_reduced_system(dict(pr, max_iters=1), lam)
        w = np.linalg.eigvalsh(S)
        assert w[0] > 0 and w[-1] / w[0] <= 3e5, w[-1] / w[0]
        xyz = W.state_after(seq["xyz"], pids, start, ref["pt_xyz"])


def test_ring_model_ignores_what_the_header_says_it_ignores():
    """quads of a negative frame, of a frame that is not in the ring, of a feature >= n; labels reset by a push; the last quad of a repeated pair holds"""
    r = W.Ring(2, 4); z = np.zeros((3, 3))
    r.push_frame(0, z, z); r.push_frame(1, z, z)
    r.set_labels([(-1, 0, 5, 0), (2, 0, 5, 0), (1, 3, 5, 0), (1, -1, 5, 0), (1, 2, 7, 1), (1, 2, 8, 2)])
    assert r.trk[1].tolist() == [-1, -1, 8] and r.pos[1].tolist() == [0, 0, 2] and r.trk[0].tolist() == [-1, -1, -1]
    r.push_frame(3, z[:2], z[:2])
    assert r.trk[1].tolist() == [-1, -1] and not r.has(1) and r.has(3) and r.has(0)
