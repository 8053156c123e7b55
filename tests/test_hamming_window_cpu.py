"""The numpy statement of vido_hamming_match_window (tests/refimpl/hamming_window_np.py) itself, on hand-made cases whose answers are written out; the array form that
tools/measure_descriptor_recover.py sweeps with, held against the statement; and the built library exporting the op and the Verify.Recover read-back.  No GPU."""
import ctypes
import importlib.util
import os
import sys
import numpy as np
import pytest

from refimpl.hamming_window_np import hamming, match_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(*bits):
    """a 256-bit descriptor with the given bits set"""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= 1 << (b % 8)
    return d


def _call(qd, qxy, ql, td, txy, tl, radius, **kw):
    return [a.tolist() for a in match_window(np.array(qd, np.uint8).reshape(-1, 32), np.array(qxy, np.float32).reshape(-1, 2), np.array(ql, np.int32),
                                             np.array(td, np.uint8).reshape(-1, 32), np.array(txy, np.float32).reshape(-1, 2), np.array(tl, np.int32), radius, **kw)]


def test_hamming_counts_bits():
    assert hamming(_desc(), _desc()) == 0 and hamming(_desc(0, 7, 8, 255), _desc(7)) == 3 and hamming(np.full(32, 255, np.uint8), _desc()) == 256


def test_a_tie_takes_the_lower_index():
    idx, dist, dist2, status, stats = _call([_desc()], [[5, 5]], [0], [_desc(1, 2, 3), _desc(9), _desc(200), _desc(4, 5)], [[5, 5]] * 4, [0] * 4, 1.0)
    assert idx == [1] and dist == [1] and dist2 == [1] and status == [0] and stats == [1, 0, 0, 0, 0]


def test_a_duplicate_descriptor_fails_any_ratio():
    td = [_desc(1, 2), _desc(1, 2), _desc(1, 2, 3, 4, 5, 6)]
    for ratio, want in ((None, 0), ((1, 1), 3), ((819, 1024), 3), ((1, 1024), 3)):
        idx, dist, dist2, status, stats = _call([_desc()], [[0, 0]], [2], td, [[0, 0]] * 3, [2] * 3, 0.0, ratio=ratio)
        assert dist == [2] and dist2 == [2] and status == [want] and idx == [0 if want == 0 else -1], ratio
    # also when the duplicate IS the query: 0 * den < 0 * num is false
    idx, dist, dist2, status, _ = _call([_desc(7)], [[0, 0]], [0], [_desc(7), _desc(7)], [[0, 0]] * 2, [0, 0], 0.0, ratio=(1, 1))
    assert dist == [0] and dist2 == [0] and status == [3] and idx == [-1]
    # a single candidate has no second: the ratio test does not apply
    idx, dist, dist2, status, _ = _call([_desc(7)], [[0, 0]], [0], [_desc(7)], [[0, 0]], [0], 0.0, ratio=(1, 1024))
    assert dist == [0] and dist2 == [-1] and status == [0] and idx == [0]
    # 819 / 1024: 4 * 1024 = 4096 < 5 * 819 = 4095 is false, 4 * 1024 < 6 * 819 = 4914 is true
    for second, want in ((5, 3), (6, 0)):
        _, dist, dist2, status, _ = _call([_desc()], [[0, 0]], [0], [_desc(0, 1, 2, 3), _desc(*range(10, 10 + second))], [[0, 0]] * 2, [0, 0], 0.0, ratio=(819, 1024))
        assert dist == [4] and dist2 == [second] and status == [want]


def test_the_window_is_a_square_with_its_edge():
    out = np.nextafter(np.float32(12.5), np.float32(np.inf)); assert out > 12.5
    txy = [[12.5, 10], [out, 10], [10, 7.5], [12.5, 12.5], [10, np.nextafter(np.float32(7.5), np.float32(-np.inf))], [12.5, 7.5]]
    td = [_desc(0), _desc(0, 1), _desc(0, 1, 2), _desc(0, 1, 2, 3), _desc(), _desc(0, 1, 2, 3, 4)]
    cand = []
    for j in range(6):                                       # one train entry at a time: is it a candidate?
        _, dist, _, status, _ = _call([_desc()], [[10, 10]], [0], [td[j]], [txy[j]], [0], 2.5)
        cand.append(status == [0])
    assert cand == [True, False, True, True, False, True]    # the corners of the square are inside (a disc of 2.5 would leave them out)
    idx, dist, dist2, status, _ = _call([_desc()], [[10, 10]], [0], td, txy, [0] * 6, 2.5)
    assert idx == [0] and dist == [1] and dist2 == [3]       # entry 4 (distance 0) and entry 1 (distance 2) are outside


def test_the_level_gate():
    td = [_desc(0), _desc(0, 1), _desc(0, 1, 2)]; lv = [3, 4, 6]
    for tol, want in ((-1, (0, 1, 2)), (0, (1, 2, -1)), (1, (0, 1, 2)), (2, (0, 1, 2))):
        idx, dist, dist2, _, _ = _call([_desc()], [[0, 0]], [4], td, [[0, 0]] * 3, lv, 1.0, level_tol=tol)
        assert (idx[0], dist[0], dist2[0]) == want, tol
    idx, dist, dist2, status, _ = _call([_desc()], [[0, 0]], [1], td, [[0, 0]] * 3, lv, 1.0, level_tol=1)
    assert (idx, dist, dist2, status) == ([-1], [-1], [-1], [1])


def test_nan_and_inf_positions_have_no_candidates():
    td = [_desc(), _desc(1)]; txy = [[1, 1], [2, 2]]
    for q in ([np.nan, 1], [1, np.nan], [np.inf, 1], [1, -np.inf]):
        idx, dist, dist2, status, stats = _call([_desc()], [q], [0], td, txy, [0, 0], 1e30)
        assert (idx, dist, dist2, status, stats) == ([-1], [-1], [-1], [1], [0, 1, 0, 0, 0]), q
    # ... and a NaN / inf train entry is nobody's candidate
    idx, dist, dist2, status, _ = _call([_desc()], [[1, 1]], [0], td + [_desc(2)], [[np.nan, 1], [np.inf, 1], [1, 1]], [0, 0, 0], 1e30)
    assert (idx, dist, dist2, status) == ([2], [1], [-1], [0])


def test_max_dist_comes_before_the_ratio():
    idx, dist, dist2, status, stats = _call([_desc()], [[0, 0]], [0], [_desc(0, 1, 2), _desc(0, 1, 2)], [[0, 0]] * 2, [0, 0], 0.0, max_dist=2, ratio=(1, 1))
    assert status == [2] and idx == [-1] and dist == [3] and dist2 == [3] and stats == [0, 0, 1, 0, 0]
    assert _call([_desc()], [[0, 0]], [0], [_desc(0, 1, 2)], [[0, 0]], [0], 0.0, max_dist=3)[3] == [0]
    assert _call([_desc()], [[0, 0]], [0], [_desc()], [[0, 0]], [0], 0.0, max_dist=0)[3] == [0]
    assert _call([_desc()], [[0, 0]], [0], [_desc()], [[0, 0]], [0], 0.0, max_dist=-1)[3] == [2]


def test_three_queries_claim_one_train_entry():
    # train 0 is everybody's best; train 1 is a worse candidate of all three: a loser does NOT fall back to it
    td = [_desc(0, 1, 2), _desc(*range(100, 140))]; txy = [[0, 0], [0, 0]]
    qd = [_desc(0, 1, 2, 3, 4, 5, 6, 7), _desc(0, 1, 2, 3, 4, 5), _desc(0, 1, 2, 9, 10, 11), _desc(*range(100, 140))]
    idx, dist, dist2, status, stats = _call(qd, [[0, 0]] * 4, [0] * 4, td, txy, [0, 0], 1.0, unique=True)
    assert dist == [5, 3, 3, 0] and status == [4, 0, 4, 0] and idx == [-1, 0, -1, 1] and stats == [2, 0, 0, 0, 2]      # equal distances: the smaller i keeps it
    idx, _, _, status, stats = _call(qd, [[0, 0]] * 4, [0] * 4, td, txy, [0, 0], 1.0, unique=False)
    assert status == [0, 0, 0, 0] and idx == [0, 0, 0, 1] and stats == [4, 0, 0, 0, 0]
    # a query that failed an earlier test does not take part in the claim: with max_dist = 4 query 0 is out before, and the claim is between 1 and 2 as before
    idx, _, _, status, stats = _call(qd, [[0, 0]] * 4, [0] * 4, td, txy, [0, 0], 1.0, max_dist=4, unique=True)
    assert status == [2, 0, 4, 0] and idx == [-1, 0, -1, 1] and stats == [2, 0, 1, 0, 1]
    # the ratio comes before the claim too: 1 / 1024 fails everybody who has a second candidate, and nobody claims
    idx, _, _, status, _ = _call(qd[:3], [[0, 0]] * 3, [0] * 3, td, txy, [0, 0], 1.0, ratio=(1, 1024), unique=True)
    assert status == [3, 3, 3] and idx == [-1, -1, -1]


def test_empty_sets_and_bad_arguments():
    e = np.zeros((0, 32), np.uint8); exy = np.zeros((0, 2), np.float32); el = np.zeros(0, np.int32)
    idx, dist, dist2, status, stats = match_window(e, exy, el, [_desc()], [[0, 0]], [0], 1.0)
    assert len(idx) == len(dist) == len(dist2) == len(status) == 0 and stats.tolist() == [0] * 5
    idx, dist, dist2, status, stats = match_window([_desc(), _desc(1)], [[0, 0], [1, 1]], [0, 0], e, exy, el, 1.0, unique=True)
    assert idx.tolist() == [-1, -1] and dist.tolist() == [-1, -1] and dist2.tolist() == [-1, -1] and status.tolist() == [1, 1] and stats.tolist() == [0, 2, 0, 0, 0]
    for bad in ((0, 1), (2, 1), (1, 1025), (-1, 4), (1025, 1025)):
        with pytest.raises(ValueError):
            match_window(e, exy, el, e, exy, el, 1.0, ratio=bad)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            match_window(e, exy, el, e, exy, el, bad)


def test_the_tools_array_form_equals_the_statement():
    spec = importlib.util.spec_from_file_location("measure_descriptor_recover", os.path.join(ROOT, "tools", "measure_descriptor_recover.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    r = np.random.default_rng(5)
    nq, nt = 150, 120
    base = r.integers(0, 256, (12, 32), dtype=np.uint8)                # a few families of near-duplicates, so that small distances, ties and claims occur
    def fam(n):
        d = base[r.integers(0, 12, n)].copy()
        for i in range(n):
            for b in r.integers(0, 256, r.integers(0, 6)):
                d[i, b // 8] ^= 1 << (b % 8)
        return d
    qd, td = fam(nq), fam(nt)
    qxy = r.integers(0, 24, (nq, 2)).astype(np.float32) / 2; txy = r.integers(0, 24, (nt, 2)).astype(np.float32) / 2
    ql = r.integers(0, 4, nq).astype(np.int32); tl = r.integers(0, 4, nt).astype(np.int32)
    D = tool.distance_matrix(qd, td)
    assert D[3, 5] == hamming(qd[3], td[5])
    seen = set()
    for radius, tol, md, ratio, uniq in ((2.0, 1, 256, None, True), (3.5, 0, 6, (819, 1024), True), (1.0, -1, 4, (922, 1024), False), (0.0, 1, 256, (1, 1), True)):
        want = match_window(qd, qxy, ql, td, txy, tl, radius, tol, md, ratio, uniq)
        got = tool.match_dense(D, qxy, ql, txy, tl, radius, tol, md, ratio, uniq)
        for a, b in zip(got, want[:4]):
            assert np.array_equal(a, b)
        seen |= set(want[3].tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_the_library_exports_the_op_and_the_read_back():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vido_slam_amd
    lib = ctypes.CDLL(vido_slam_amd.LIB_PATH)
    for name in ("vido_hamming_match_window", "vido_system_get_recover_points", "vido_system_get_recover_stats"):
        assert hasattr(lib, name), name
    from vido_slam_amd.host import Context
    from vido_slam_amd.system import System
    assert hasattr(Context, "hamming_match_window") and hasattr(Context, "hamming_match_window_device")
    assert hasattr(System, "recover_points") and hasattr(System, "recover_stats")
