"""Direct tests of the device-resident local-BA window (csrc/bawin.hip): the ring, the graph assembly, the solve on device inputs and the write-back.

Reference: tests/refimpl/bawin_np.py (plain numpy; its own consistency and the preconditions of the bounds below: tests/test_bawin_ref_cpu.py).

A. Exact graph.  With max_iters = 0 the solver takes the host driver, evaluates chi2 and leaves the assembled landmarks alone, so k_bawin_writeback stores into every
   observation row the f32 xyz of the feature that started its chain, unchanged to the bit.  Every pushed xyz row is distinct, so read_points tells per feature which chain
   it was attached to; a feature that keeps its own row was given no landmark.  After every solve of a sliding window: graph sizes = the Map walk's, no iteration or trial
   counted, cam_T returned bit-identical, chi2_final == chi2_initial, |chi2_initial - oracle.ba_chi2(walk problem)| <= max(1e-12, n_terms * 2^-52) * chi2 (all terms are
   non-negative: the worst case of any summation order; n_terms = observations + odometry factors + prior), and read_points of every frame in the ring bit-equal to the model.
B. Hostile and edge inputs: return codes, messages and the exact state after a following zero-iteration solve.
C. Solve parity at max_iters 1, 2 (4 from the hard start) with oracle.ba_optimize on the walk's problem, at the bound of tests/test_ba_step_gpu.py:
   |got - ref| <= 1e-9 * step + 100 * floor on cam_T, (iterations, lm_trials) equal, chi2_initial / chi2_final / lambda_final at 1e-9 relative, the `[ba] path:` line says
   `driver resident`; every observation row of read_points within bound + one f32 ulp of f32(reference landmark) (the ulp: a rounding flip at the cast), every other row
   bit-equal to what was pushed; then the window slides by one frame and the second solve is compared with a reference built from the state read back from the ring.

Not tested: the VIDO_E_CAPACITY return of vido_bawin_solve.  cap_obs = cap_pt = cap_frames * cap_features and a window is shorter than the ring, so a window never holds more
observations or landmarks than the tables have rows: the branch cannot be reached through the API.

Observed on the MI355X.

A (graph sizes are (landmarks, observations); a stream's first two windows are empty graphs, a tracklet being labelled with its third frame):
  scenario    ring (frames x features), window   windows  largest graph     graphs with landmarks   largest |chi2 - ref| / chi2   (bound)
  tiny        4 x 6, 3                           10       (3, 9)            4                       2.2e-16                       1e-12
  ipt_edges   5 x 2100, 4                        12       (996, 3074)       7                       2.5e-15                       1e-12
  production  24 x 8192, 20                      26       (23924, 106608)   24                      9.8e-15                       2.4e-11 at 106 k terms
  one_camera  4 x 300, 1                         4 + 4    (147, 147)        2                       2.5e-16                       1e-12
  tiny: frames of 2, 4, 6, 6, 0, 3, 5, 6, 1, 6 features; a window of 3 holds only the tracklets born in its first frame that are 3 long, so its graphs have 1-3 landmarks.
  one_camera: the four windows at the head are empty graphs (see bawin_np.SCENARIOS), the windows [0, 1) and [1, 2) solved after the last push hold 147 and 21 landmarks.
  read_points was bit-equal to the model after every one of the 56 solves, in every frame of the ring.

C (err = max |got - ref| over cam_T; bound = 1e-9 * step + 100 * floor; the write-back error of every observation row was 0: f32(landmark) = f32(reference landmark)):
  case         k  window  (it,tr)  landmarks  obs   step    floor    bound     err       err/bound
  w5           1  1       (1, 1)   55         267   0.0643  8.3e-17  6.44e-11  1.1e-16   1.7e-06
  w5           1  2       (1, 1)   4          17    0.0379  1.1e-16  3.79e-11  1.1e-16   2.9e-06
  w5           2  1       (2, 2)   55         267   0.0949  4.4e-16  9.5e-11   4.4e-16   4.7e-06
  w5           2  2       (2, 2)   4          17    0.0874  2.8e-17  8.75e-11  5.6e-17   6.3e-07
  w20_prior    1  1       (1, 1)   198        2027  0.107   3.1e-16  1.07e-10  1.4e-16   1.3e-06
  w20_prior    1  2       (1, 1)   113        944   0.0996  1.8e-16  9.96e-11  1.1e-16   1.1e-06
  w20_prior    2  1       (2, 2)   198        2027  0.138   1.1e-16  1.38e-10  2.2e-16   1.6e-06
  w20_prior    2  2       (2, 2)   113        944   0.138   2.2e-16  1.38e-10  2.2e-16   1.6e-06
  w20_free     1  1       (1, 1)   198        2027  0.456   1.3e-14  4.57e-10  1.1e-14   2.4e-05
  w20_free     1  2       (1, 1)   113        944   0.84    1.4e-14  8.41e-10  1.6e-14   1.9e-05
  w20_free     2  1       (2, 2)   198        2027  1.11    7.8e-14  1.12e-09  1.1e-13   9.7e-05
  w20_free     2  2       (2, 2)   113        944   0.87    2.9e-13  8.99e-10  3.1e-13   0.00035
  w20_hard     2  1       (2, 5)   187        2034  17.4    2.5e-11  1.99e-08  2.6e-11   0.0013
  w20_hard     2  2       (2, 3)   96         826   14.1    3.3e-12  1.44e-08  2.7e-12   0.00019
  w20_hard     4  1       (4, 7)   187        2034  13.9    2.5e-11  1.64e-08  2.5e-11   0.0015
  w20_hard     4  2       (4, 6)   96         826   11.2    5.7e-12  1.18e-08  5.1e-12   0.00043
The device-inputs route sits at the floor of the two CPU algorithms like the host-inputs route does; the zero-iteration behaviour of the host-inputs route
(tests/test_ba_step_gpu.py::test_zero_iterations_return_the_input) holds for device inputs too, the one-camera window included.  The module runs in 2 s.

The tests fail on a kernel that is subtly wrong.  One-line mutations of csrc/bawin.hip that keep every index in range, built as variant libraries and run once each against
this module (22 tests):
  * k_bawin_ingest without the `trk = -1` reset                -> 4 fail: A tiny, ipt_edges, production; the reused-slot test
  * k_bawin_labels addressing slot (frame + 1) % cap_f         -> 21 fail: everything but the empty-graph test
  * k_bawin_assemble: is_new for `ps <= 0`                     -> 1 fails: the negative-position test (added for this mutation: no other input carries a position < 0)
  * k_bawin_assemble: meas copied with x and y swapped         -> 12 fail: A (all four, by chi2), C (all eight)
  * k_bawin_assemble: landmark initialised from xyz[3 * o] x 3 -> 21 fail: everything but the empty-graph test
  * k_bawin_writeback skipping the observations of camera 0    -> 8 fail: C (all eight).  Part A cannot see it: an observation from the window's first camera starts its
                                                                  chain, and after a zero-iteration solve the row of a chain's first feature holds its own value either way
  * vido_bawin_set_labels without the one-quad-per-pair staging (the code before this test existed) -> 0 fail on the run made: the unordered stores of k_bawin_labels
                                                                  happened to land in list order.  Nothing guarantees that order; the test pins the rule the header now states.
"""
import ctypes as C
import re
import numpy as np
import pytest

from refimpl import bawin_np as W

pytestmark = pytest.mark.gpu
PATH_RE = re.compile(r"\[ba\] path: schur (\w+) schur_long (\d+) \| solver (\w+) \| driver (\w+)")
E_INVALID, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=640, height=480, max_batch=1)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_points(win, model, frames, tag):
    """read_points of every listed frame bit-equal to the model"""
    for f in frames:
        want = model.read_points(f); got = win.read_points(f, len(want))
        bad = np.nonzero(np.any(_bits(got) != _bits(want), axis=1))[0]
        assert len(bad) == 0, "%s: frame %d, %d of %d rows differ, first: feature %d got %s want %s" % (tag, f, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def _zero_result(got, pr):
    assert got["n_obs"] == 0 and got["n_pt"] == 0 and got["iterations"] == 0 and got["lm_trials"] == 0
    assert got["chi2_initial"] == 0 and got["chi2_final"] == 0 and got["lambda_final"] == 0
    assert np.array_equal(got["cam_T"], np.asarray(pr["cam_T"]))


# ---- A ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", list(W.SCENARIOS))
def test_exact_graph_over_a_sliding_window(vido, oracle, ctx, sid):
    sc, seq, labels, _, deliveries = W.scenario(sid)
    win = vido.BaWindow(ctx, sc["cap_f"], sc["cap_n"]); model = W.Ring(sc["cap_f"], sc["cap_n"])
    pushed = 0; worst = 0.0; sizes = []
    for upto, start, N in W.windows(sc):
        while pushed < upto:
            a = seq["asso"][pushed] if pushed else None
            win.push_frame(pushed, seq["meas"][pushed], seq["xyz"][pushed], a); model.push_frame(pushed, seq["meas"][pushed], seq["xyz"][pushed], a)
            win.set_labels(deliveries[pushed]); model.set_labels(deliveries[pushed]); pushed += 1
        in_ring = [f for f in range(pushed) if model.has(f)]
        state = [model.read_points(f) if model.has(f) else seq["xyz"][f] for f in range(seq["n_frames"])]
        pr, pids = W.walk(seq, labels, start, N, xyz=state, prior_cam=0 if N == sc["win"] else -1, max_iters=0, upto=upto)
        got = win.solve(start, N, pr)
        status, n_obs, n_pt = model.solve0(start, N)
        tag = "%s window [%d, %d)" % (sid, start, N)
        assert status == W.VIDO_OK and (n_obs, n_pt) == (len(pr["obs_cam"]), pr["n_pt"]), tag
        assert (got["n_obs"], got["n_pt"]) == (n_obs, n_pt), (tag, got["n_obs"], got["n_pt"], n_obs, n_pt)
        sizes.append((n_pt, n_obs))
        if n_pt == 0:
            _zero_result(got, pr)
        else:
            assert got["iterations"] == 0 and got["lm_trials"] == 0, tag
            assert np.array_equal(got["cam_T"], np.asarray(pr["cam_T"])), tag
            assert got["chi2_final"] == got["chi2_initial"], tag
            chi = oracle.ba_chi2(pr); n_terms = n_obs + len(pr["odo_i"]) + (1 if pr["prior_cam"] >= 0 else 0)
            dev = abs(got["chi2_initial"] - chi) / chi; worst = max(worst, dev)
            assert dev <= max(1e-12, n_terms * 2.0 ** -52), (tag, got["chi2_initial"], chi, dev)
        _same_points(win, model, in_ring, tag)
    print("\n[bawin A] %-10s windows %d, largest graph %s (landmarks, observations), largest |chi2 - ref| / chi2 = %.2g | sizes %s" % (sid, len(sizes), max(sizes), worst, sizes))
    assert sum(1 for s in sizes if s[0]) >= 2


# ---- B ---------------------------------------------------------------------------------------------------------
def _rows(rng, n, f):
    """n features of frame f: meas, distinct xyz rows"""
    xyz = (1000.0 * f + 10.0 * np.arange(n)[:, None] + np.array([1.0, 2.0, 3.0]) + rng.uniform(0, 0.5, (n, 3))).astype(np.float32)
    return rng.normal(0, 1, (n, 3)) + np.array([0, 0, 10.0]), xyz


def _cams(vido, nc, max_iters=0):
    I = np.eye(4)[:3]
    d = dict(n_cam=nc, cam_T=np.tile(I, (nc, 1, 1)), odo_i=np.arange(nc - 1, dtype=np.int32), odo_j=np.arange(1, nc, dtype=np.int32), odo_T=np.tile(I, (max(nc - 1, 0), 1, 1)),
             prior_cam=-1, prior_T=I.copy(), max_iters=max_iters)
    c = vido.problems.ba_constants("local"); c.pop("max_iters"); d.update(c)
    return d


class _Pair:
    """the ring and its model, stepped together"""

    def __init__(self, vido, ctx, cap_f, cap_n, seed=0):
        self.vido = vido; self.win = vido.BaWindow(ctx, cap_f, cap_n); self.model = W.Ring(cap_f, cap_n); self.rng = np.random.RandomState(seed); self.pushed = {}

    def push(self, f, n, asso=None):
        meas, xyz = _rows(self.rng, n, f); a = None if asso is None else np.asarray(list(asso), np.int64)
        assert a is None or len(a) == n
        self.win.push_frame(f, meas, xyz, a); self.model.push_frame(f, meas, xyz, a); self.pushed[f] = xyz

    def labels(self, quads, model_too=True):
        self.win.set_labels(quads)
        if model_too:
            self.model.set_labels(quads)

    def solve0(self, start, N):
        """-> (n_pt, n_obs) after both agreed; raises what the library raises"""
        status, n_obs, n_pt = self.model.solve0(start, N)
        got = self.win.solve(start, N, _cams(self.vido, N - start))
        assert status == W.VIDO_OK and (got["n_obs"], got["n_pt"]) == (n_obs, n_pt), (got["n_obs"], got["n_pt"], n_obs, n_pt)
        assert got["iterations"] == 0 and got["lm_trials"] == 0 and got["chi2_final"] == got["chi2_initial"]
        _same_points(self.win, self.model, [f for f in self.pushed if self.model.has(f)], "window [%d, %d)" % (start, N))
        return n_pt, n_obs


def _chain_quads(frames, n, t0=0, p0=0):
    """identity chains over `frames`: feature j of every frame on tracklet t0 + j, position p0 + (index of the frame)"""
    return [(f, j, t0 + j, p0 + k) for k, f in enumerate(frames) for j in range(n)]


def test_duplicate_predecessor_is_invalid_and_the_ring_recovers(vido, ctx):
    P = _Pair(vido, ctx, 4, 4)
    P.push(0, 4); P.push(1, 4, [0, 1, 2, 3]); P.push(2, 4, [1, 1, 2, 3])              # features 0 and 1 of frame 2 both continue feature 1 of frame 1
    P.labels(_chain_quads([0, 1, 2], 4))
    assert P.model.assemble(0, 3)[0] == W.VIDO_E_INVALID
    with pytest.raises(vido.VidoError) as e:
        P.win.solve(0, 3, _cams(vido, 3))
    assert e.value.code == E_INVALID and "bawin_solve" in str(e.value) and "observed twice" in str(e.value)
    _same_points(P.win, P.model, [0, 1, 2], "after the refused solve")               # nothing was written back
    P.labels([(2, 0, -1, 0)])
    assert P.solve0(0, 3) == (4, 11)                                                   # chain 0 ends in frame 1; nothing left over in the per-landmark counters:
    assert P.solve0(0, 3) == (4, 11)                                                   # ... the same window assembles again, and another one too
    assert P.solve0(1, 3) == (0, 0)
    P.labels(_chain_quads([1, 2], 4, t0=20)); P.labels([(2, 0, -1, 0)])
    assert P.solve0(1, 3) == (4, 7)


def test_asso_out_of_range_drops_the_chain_and_nothing_else(vido, ctx):
    P = _Pair(vido, ctx, 5, 5)
    P.push(0, 5); P.push(1, 5, [5, 2 ** 31 - 1, -5, 3, 4]); P.push(2, 5, [0, 1, 2, 3, 4]); P.push(3, 5, [0, 1, 2, 3, 4])
    P.labels(_chain_quads([0, 1, 2, 3], 5))
    assert P.solve0(0, 4) == (5, 5 + 3 * 2)                                            # the chains through features 0, 1, 2 of frame 1 end in frame 0, their successors are dropped
    assert np.array_equal(P.win.read_points(3, 5)[:3], P.pushed[3][:3]) and np.array_equal(P.win.read_points(3, 5)[3:], P.pushed[0][3:])
    assert P.solve0(1, 4) == (0, 0)


def test_a_reused_slot_starts_without_labels_and_stale_ids_do_not_leak(vido, ctx):
    P = _Pair(vido, ctx, 4, 5)
    P.push(0, 5); P.push(1, 5, range(5)); P.push(2, 5, range(5)); P.push(3, 5, range(5))
    P.labels(_chain_quads([0, 1, 2], 5))
    assert P.solve0(0, 3) == (5, 15)                                                   # (leaves landmark ids in the id rows of slot 0, and slot 0 labelled at position 0)
    P.labels(_chain_quads([2, 3], 5, t0=10))                                           # frame 2 re-labelled: position 0 of new tracklets
    P.push(4, 3, [0, 1, 2])                                                            # takes slot 0 with fewer features; no quads for it
    assert P.solve0(2, 5) == (5, 10)                                                   # no landmark in frame 4, the chains end in frame 3
    assert np.array_equal(P.win.read_points(4, 3), P.pushed[4])
    P.push(5, 5, [0, 1, 2, 3, 4]); P.labels(_chain_quads([5], 5, t0=10, p0=3))          # features 3, 4 point past frame 4's three features, at the stale rows of frame 0
    assert P.solve0(3, 6) == (0, 0)
    with pytest.raises(vido.VidoError) as e:
        P.win.read_points(4, 4)
    assert e.value.code == E_INVALID and "bawin_read_points" in str(e.value)


def test_null_asso_means_unassociated(vido, ctx):
    P = _Pair(vido, ctx, 4, 5)
    P.push(0, 5); P.push(1, 5); P.push(2, 5, range(5))
    P.labels(_chain_quads([0, 1, 2], 5))
    assert P.solve0(0, 3) == (5, 5)
    assert P.solve0(1, 3) == (0, 0)


def test_a_labelled_feature_at_a_negative_position_has_no_landmark(vido, ctx):
    """neither the start of a landmark (position 0) nor a continuation (position > 0): the feature and its successors are left out"""
    P = _Pair(vido, ctx, 4, 5)
    P.push(0, 5); P.push(1, 5, range(5)); P.push(2, 5, range(5))
    P.labels(_chain_quads([0, 1, 2], 5)); P.labels([(0, 1, 1, -1), (1, 3, 3, -1), (1, 4, 4, -(2 ** 31))])
    assert P.solve0(0, 3) == (4, 4 + 2 + 2)


def test_a_window_without_labels_is_an_empty_graph(vido, ctx):
    P = _Pair(vido, ctx, 4, 5)
    P.push(0, 5); P.push(1, 5, range(5)); P.push(2, 0, []); P.push(3, 2)
    pr = _cams(vido, 3); pr["cam_T"] = pr["cam_T"] + 0.125
    _zero_result(P.win.solve(0, 3, pr), pr)
    _zero_result(P.win.solve(2, 4, _cams(vido, 2)), _cams(vido, 2))
    _same_points(P.win, P.model, [0, 1, 2, 3], "no labels")


def test_quads_that_must_be_ignored(vido, ctx):
    P = _Pair(vido, ctx, 3, 6)
    for f in range(5):
        P.push(f, 4 if f != 3 else 2, None if f == 0 else [0, 1, 2, 3][:4 if f != 3 else 2])
    good = _chain_quads([2, 3, 4], 2, p0=0)
    junk = [(-1, 0, 50, 0), (-3, 1, 50, 0), (0, 0, 50, 0), (1, 1, 50, 0), (5, 0, 50, 0), (8, 0, 50, 0), (3, 2, 50, 0), (3, 3, 50, 0), (4, 4, 50, 0), (4, 5, 50, 0), (4, 6, 50, 0),
            (4, -1, 50, 0), (4, 2 ** 31 - 1, 50, 0), (2, -(2 ** 31), 50, 0), (2 ** 31 - 1, 0, 50, 0)]
    mixed = [q for pair in zip(junk, good + good + good) for q in pair]
    P.labels(mixed, model_too=False); P.model.set_labels(good)                        # the model never sees the junk
    assert P.solve0(2, 4) == (2, 4)
    P.labels(junk)
    assert P.solve0(3, 5) == (0, 0) and P.solve0(2, 4) == (2, 4)


def test_more_quads_than_one_staging_chunk(vido, ctx):
    """cap_features = 4: a chunk stages 26 quads.  200 quads in one call (188 that must not survive, then the 12 that hold) = the same quads one per call."""
    wrong = [(f, j, 99, 0) if (i // 12) % 2 else (f, j, -1, 3) for i in range(188) for f, j in [((i % 12) // 4, i % 4)]]
    quads = wrong + _chain_quads([0, 1, 2], 4)
    assert len(quads) == 200
    out = []
    for one_call in (True, False):
        P = _Pair(vido, ctx, 4, 4, seed=1)
        P.push(0, 4); P.push(1, 4, [1, 0, 3, 2]); P.push(2, 4, [3, 2, 1, 0])
        if one_call:
            P.labels(quads)
        else:
            for q in quads:
                P.labels([q])
        assert P.solve0(0, 3) == (4, 12)
        out.append([P.win.read_points(f, 4) for f in range(3)])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*out))


def test_the_last_quad_of_a_repeated_pair_holds(vido, ctx):
    """512 (frame, feature) pairs occur twice in one call, the two quads 1536 positions apart.  The first quad of the even features carries the larger position value and
    no tracklet (the feature would have no landmark), the first quad of the odd ones the smaller position value (the feature would start a landmark of its own)."""
    n = 512; P = _Pair(vido, ctx, 4, n)
    perm = np.random.RandomState(3).permutation(n)
    P.push(0, n); P.push(1, n, perm); P.push(2, n, perm)
    first = [(1, j, -1, 5) if j % 2 == 0 else (1, j, 1000 + j, 0) for j in range(n)]
    last = [(1, j, 7, 1) for j in range(n)]
    quads = first + _chain_quads([0], n) + [(2, j, 7, 2) for j in range(n)] + last
    assert all(quads.index(last[j]) - quads.index(first[j]) > 256 for j in (0, 1, n - 2, n - 1))
    P.labels(quads)
    assert P.solve0(0, 3) == (n, 3 * n)


def test_argument_checks(vido, ctx):
    from vido_slam_amd import host as H
    lib, h = ctx.lib, ctx.h
    fresh = vido.Context(width=640, height=480, max_batch=1)
    try:                                                                               # every call before create
        z = np.zeros((2, 3)); zf = np.zeros((2, 3), np.float32); q = np.zeros((1, 4), np.int32); pr = _cams(vido, 1)
        p, keep = H._ba_problem_struct(pr, graph=False); r = H.BaResult()
        calls = {"bawin_push_frame": lambda c: c.lib.vido_bawin_push_frame(c.h, 0, 2, z.ctypes.data, zf.ctypes.data, None),
                 "bawin_set_labels": lambda c: c.lib.vido_bawin_set_labels(c.h, 1, q.ctypes.data),
                 "bawin_solve": lambda c: c.lib.vido_bawin_solve(c.h, 0, 1, C.byref(p), C.byref(r), None, None),
                 "bawin_read_points": lambda c: c.lib.vido_bawin_read_points(c.h, 0, 2, zf.ctypes.data)}
        for name, call in calls.items():
            assert call(fresh) == E_INVALID and name in fresh.lib.vido_last_error(fresh.h).decode(), name
    finally:
        fresh.close()

    def refused(code, name, fn, *a):
        with pytest.raises(vido.VidoError) as e:
            fn(*a)
        assert e.value.code == code and name in str(e.value), (code, name, str(e.value))
    for cf, cn in ((1, 8), (65, 8), (4, 0), (4, 8193)):
        refused(E_INVALID, "bawin_create", vido.BaWindow, ctx, cf, cn)
    P = _Pair(vido, ctx, 4, 3)
    meas, xyz = _rows(P.rng, 4, 0)
    refused(E_CAPACITY, "bawin_push_frame", P.win.push_frame, 0, meas, xyz)
    refused(E_INVALID, "bawin_push_frame", P.win.push_frame, -1, meas[:2], xyz[:2])
    assert lib.vido_bawin_push_frame(h, 0, -1, meas.ctypes.data, xyz.ctypes.data, None) == E_INVALID and "bawin_push_frame" in lib.vido_last_error(h).decode()
    for f in range(6):
        P.push(f, 3 if f != 4 else 2, None if f == 0 else [0, 1, 2][:3 if f != 4 else 2])
    P.labels(_chain_quads([3, 4, 5], 2))
    refused(E_INVALID, "bawin_solve", P.win.solve, 4, 4, _cams(vido, 1))              # N <= start
    refused(E_INVALID, "bawin_solve", P.win.solve, 5, 4, _cams(vido, 1))
    refused(E_INVALID, "bawin_solve", P.win.solve, 2, 6, _cams(vido, 4))              # N - start >= cap_frames
    refused(E_INVALID, "bawin_solve", P.win.solve, 3, 6, _cams(vido, 2))              # n_cam != N - start
    refused(E_INVALID, "bawin_solve", P.win.solve, 1, 4, _cams(vido, 3))              # frame 1 has left the ring
    refused(E_INVALID, "bawin_solve", P.win.solve, 5, 7, _cams(vido, 2))              # frame 6 has not arrived
    refused(E_INVALID, "bawin_solve", P.win.solve, -1, 1, _cams(vido, 2))
    refused(E_INVALID, "bawin_read_points", P.win.read_points, 1, 3)                  # departed
    refused(E_INVALID, "bawin_read_points", P.win.read_points, 4, 3)                  # more than stored
    refused(E_INVALID, "bawin_read_points", P.win.read_points, -1, 1)
    assert lib.vido_bawin_set_labels(h, -1, None) == E_INVALID and "bawin_set_labels" in lib.vido_last_error(h).decode()
    assert lib.vido_bawin_set_labels(h, 1, None) == E_INVALID
    assert P.solve0(3, 6) == (2, 6)                                                    # the refused calls changed nothing
    P.win.create(4, 3)                                                                 # a second create drops the stored frames
    refused(E_INVALID, "bawin_read_points", P.win.read_points, 5, 1)
    refused(E_INVALID, "bawin_solve", P.win.solve, 3, 6, _cams(vido, 3))


# ---- C ---------------------------------------------------------------------------------------------------------
def _solve_window(win, pr, start, N, monkeypatch, capfd):
    monkeypatch.setenv("VIDO_BA_VERBOSE", "1")
    seen = capfd.readouterr()
    got = win.solve(start, N, pr)
    m = PATH_RE.findall(capfd.readouterr().err)
    print(seen.out, end="")
    assert len(m) == 1 and m[0][3] == "resident", m
    return got


def _compare(tag, pr, pids, start, got, points, pushed_state):
    """got / points (read_points of every frame) against the two CPU solves of `pr`; prints the bound's figures"""
    R = W.references(pr); ref, ref2 = R["ref"], R["ref2"]; bound = 1e-9 * R["step"] + 100 * R["floor"]
    # the preconditions of the bound, on this very input (for the second window it exists only here)
    assert (ref["iterations"], ref["lm_trials"]) == (ref2["iterations"], ref2["lm_trials"]) and R["floor"] <= 1e-10 * R["step"], (tag, R["floor"], R["step"])
    e_cam = float(np.abs(got["cam_T"] - ref["cam_T"]).max()); e_pt = 0.0
    assert (got["n_obs"], got["n_pt"]) == (len(pr["obs_cam"]), pr["n_pt"]), tag
    assert (got["iterations"], got["lm_trials"]) == (ref["iterations"], ref["lm_trials"]), tag
    assert np.all(np.abs(got["cam_T"] - ref["cam_T"]) <= bound), (tag, e_cam, bound)
    for key in ("chi2_initial", "chi2_final", "lambda_final"):
        assert abs(got[key] - ref[key]) <= 1e-9 * abs(ref[key]), (tag, key, got[key], ref[key])
    for f in range(len(points)):
        pid = pids[f - start] if start <= f < start + len(pids) else -np.ones(len(points[f]), np.int64)
        obs = pid >= 0
        assert np.array_equal(_bits(points[f][~obs]), _bits(pushed_state[f][~obs])), (tag, f)          # every non-observation row: untouched to the bit
        want = ref["pt_xyz"][pid[obs]].astype(np.float32)
        err = np.abs(points[f][obs].astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= bound + np.spacing(np.abs(want)).astype(np.float64)), (tag, f, err.max(), bound)
        if obs.any():
            e_pt = max(e_pt, float(err.max()))
    print("\n[bawin C] %-22s (it, trials) %s | landmarks %d obs %d | step %.3g floor %.2g bound %.3g | err cam %.3g = %.2g of the bound | write-back err %.3g (f32 ulp %.2g)" % (
        tag, (got["iterations"], got["lm_trials"]), pr["n_pt"], len(pr["obs_cam"]), R["step"], R["floor"], bound, e_cam, e_cam / bound, e_pt,
        float(np.spacing(np.float32(np.abs(ref["pt_xyz"]).max())))))


@pytest.mark.parametrize("cid,max_iters", W.PARITY_RUNS, ids=["%s-%d" % r for r in W.PARITY_RUNS])
def test_solve_and_write_back_match_the_oracle_on_consecutive_windows(vido, oracle, ctx, monkeypatch, capfd, cid, max_iters):
    pc, seq, labels = W.parity_case(cid)
    win = vido.BaWindow(ctx, pc["cap_f"], pc["n"])
    state = [np.array(x) for x in seq["xyz"]]                       # what the ring holds, as verified so far
    for f in range(pc["N"]):
        win.push_frame(f, seq["meas"][f], seq["xyz"][f], seq["asso"][f] if f else None); win.set_labels(labels[f])
    for second in (False, True):
        if second:
            f = pc["N"]; win.push_frame(f, seq["meas"][f], seq["xyz"][f], seq["asso"][f]); win.set_labels(labels[f])
        pr, pids, (start, N) = W.parity_problem(cid, max_iters, second=second, xyz=state)
        got = _solve_window(win, pr, start, N, monkeypatch, capfd)
        points = [win.read_points(f, seq["n"][f]) for f in range(N)]
        _compare("%s-%d window %d" % (cid, max_iters, 1 + second), pr, pids, start, got, points, state)
        if pc["hard"] and not second:
            assert got["lm_trials"] > got["iterations"]            # trials were rejected, on the resident driver
        state = points + state[N:]
