"""The numpy statement of vido_stereo_filter (tests/refimpl/stereo_filter_np.py) against a literal flood fill, against mask_components_np as an independent labelling,
on the inputs that show the edge relation is not transitive, at its parameter edges, on the SGM statement's output and on its quality bar.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refimpl import mask_components_np as CC                                  # noqa: E402
from refimpl import stereo_filter_cases as CASES                              # noqa: E402
from refimpl import stereo_filter_np as F                                     # noqa: E402

FLT_MAX_BITS = 0x7F7FFFFF


def flood_fill(q4, status, max_diff_q4, min_region, bf=None):
    """The rule read literally: Python integers, one pixel at a time, an explicit stack.  -> (disp, status_out, depth, stats, area per pixel)"""
    q = np.asarray(q4).tolist(); s = np.asarray(status).tolist()
    h, w = len(q), len(q[0])
    ok = [[s[y][x] == 0 and 1 <= q[y][x] <= 65535 for x in range(w)] for y in range(h)]
    out = [[(3 if s[y][x] == 0 and not ok[y][x] else s[y][x]) for x in range(w)] for y in range(h)]
    area = [[0] * w for _ in range(h)]
    seen = [[False] * w for _ in range(h)]
    regions = pixels = 0
    for y0 in range(h):
        for x0 in range(w):
            if not ok[y0][x0] or seen[y0][x0]:
                continue
            seen[y0][x0] = True; stack = [(y0, x0)]; members = []
            while stack:
                y, x = stack.pop(); members.append((y, x))
                for ny, nx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= ny < h and 0 <= nx < w and ok[ny][nx] and not seen[ny][nx] and abs(q[y][x] - q[ny][nx]) <= max_diff_q4:
                        seen[ny][nx] = True; stack.append((ny, nx))
            for y, x in members:
                area[y][x] = len(members)
            if len(members) < min_region:
                regions += 1; pixels += len(members)
                for y, x in members:
                    out[y][x] = 4
    disp = np.full((h, w), -1, np.float32); depth = None if bf is None else np.full((h, w), F.FLT_MAX, np.float32)
    for y in range(h):
        for x in range(w):
            if out[y][x] == 0:
                disp[y, x] = q[y][x] / 16.0
                if bf is not None:
                    depth[y, x] = np.float32(bf) / np.float32(q[y][x] / 16.0)
    n_in = sum(map(sum, ok))
    return disp, np.array(out, np.uint8), depth, np.array([n_in, regions, pixels, n_in - pixels], np.int32), np.array(area, np.int64)


def same(got, want):
    for g, w_, name in zip(got, want, ("disp", "status", "depth", "stats")):
        if w_ is None:
            assert g is None, name
            continue
        assert g.dtype == w_.dtype and g.shape == w_.shape, name
        assert g.tobytes() == w_.tobytes(), name


# ---- (a) the literal flood fill ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES.random_cases(), ids=lambda c: c[0])
def test_statement_equals_flood_fill(case):
    name, q4, status, params, shows = case
    assert shows(F), "the case is not what its name says"
    for p in (params, dict(max_diff_q4=0, min_region=2), dict(max_diff_q4=40, min_region=30), dict(max_diff_q4=65535, min_region=1)):
        want = flood_fill(q4, status, p["max_diff_q4"], p["min_region"], bf=75.0)
        same(F.stereo_filter(q4, status, bf=75.0, **p), want[:4])
        assert np.array_equal(F.region_areas(q4, status, p["max_diff_q4"])[1], want[4])


# ---- (b) mask_components_np as an independent labelling ---------------------------------------------
@pytest.mark.parametrize("case", CASES.pattern_cases(), ids=lambda c: c[0])
def test_constant_disparity_regions_are_4_connected_components(case):
    name, q4, status, params, shows = case
    assert shows(F), "the validity mask is not the pattern"
    v = F.valid(q4, status)
    A = CC.anchors(v.astype(np.int32), connectivity=4)
    cnt = np.bincount(A[A >= 0], minlength=A.size + 1)
    area = np.where(A >= 0, cnt[np.maximum(A, 0)], 0)
    got_A, got_area = F.region_areas(q4, status, params["max_diff_q4"])
    assert np.array_equal(got_A, A) and np.array_equal(got_area, area)
    _, st, _, stats = F.stereo_filter(q4, status, **params)
    removed = v & (area < params["min_region"])
    assert np.array_equal(st == 4, removed)
    assert stats.tolist() == [int(v.sum()), len(np.unique(A[removed])), int(removed.sum()), int(v.sum() - removed.sum())]
    assert np.array_equal(st[~v], np.where(status[~v] == 0, 3, status[~v]))


# ---- (c) the relation is not transitive -------------------------------------------------------------
def test_column_ramp_is_one_region_at_16_and_columns_at_15():
    q4, status = CASES.column_ramp(); h, w = q4.shape
    assert q4[0, -1] - q4[0, 0] == 16 * (w - 1) > 16
    A, area = F.region_areas(q4, status, 16)
    assert (A == 0).all() and (area == h * w).all()
    A, area = F.region_areas(q4, status, 15)
    assert len(np.unique(A)) == w and (area == h).all() and np.array_equal(A, np.broadcast_to(np.arange(w), (h, w)))
    assert F.stereo_filter(q4, status, 16, h * w)[3].tolist() == [h * w, 0, 0, h * w]
    assert F.stereo_filter(q4, status, 15, h + 1)[3].tolist() == [h * w, w, h * w, 0]
    assert F.stereo_filter(q4, status, 15, h)[3].tolist() == [h * w, 0, 0, h * w]


def test_boustrophedon_ramp_is_one_region_through_the_path_only():
    q4, status = CASES.boustrophedon(97, 130)
    r, d = F.edges(q4, status, 1)
    assert not r.any() and not d.any()                               # the property: at max_diff_q4 = 1 there are no edges at all
    r, d = F.edges(q4, status, 2)
    assert r.all() and d.sum() == 96                                 # every horizontal step, and one vertical step per row pair: a path, nothing else
    A, area = F.region_areas(q4, status, 2)
    assert (A == 0).all() and (area == 12610).all()
    assert F.stereo_filter(q4, status, 2, 12610)[3].tolist() == [12610, 0, 0, 12610]
    assert F.stereo_filter(q4, status, 2, 12611)[3].tolist() == [12610, 1, 12610, 0]
    assert F.stereo_filter(q4, status, 1, 2)[3].tolist() == [12610, 12610, 12610, 0]


@pytest.mark.parametrize("case", CASES.ramp_cases(), ids=lambda c: c[0])
def test_ramp_cases_equal_flood_fill(case):
    name, q4, status, params, shows = case
    assert shows(F)
    same(F.stereo_filter(q4, status, bf=3.5, **params), flood_fill(q4, status, params["max_diff_q4"], params["min_region"], bf=3.5)[:4])


# ---- (d) parameter edges ----------------------------------------------------------------------------
def test_min_region_edges():
    q4 = np.full((9, 11), 80, np.int32); status = np.zeros((9, 11), np.uint8)
    status[:, 5] = 1                                                 # two regions: 9 x 5 = 45 pixels each
    for m, gone in ((1, 0), (45, 0), (46, 90), (1 << 24, 90)):
        disp, st, depth, stats = F.stereo_filter(q4, status, 0, m)
        assert stats.tolist() == [90, 2 if gone else 0, gone, 90 - gone] and depth is None
        assert ((st == 4).sum(), (st == 1).sum()) == (gone, 9)
    with pytest.raises(ValueError):
        F.stereo_filter(q4, status, 0, 0)
    with pytest.raises(ValueError):
        F.stereo_filter(q4, status, 0, (1 << 24) + 1)


def test_max_diff_edges():
    q4 = np.array([[1, 65535, 1, 1, 2]], np.int32); status = np.zeros((1, 5), np.uint8)
    assert F.region_areas(q4, status, 0)[1].tolist() == [[1, 1, 2, 2, 1]]
    assert F.region_areas(q4, status, 65533)[1].tolist() == [[1, 1, 3, 3, 3]]
    assert F.region_areas(q4, status, 65534)[1].tolist() == [[5] * 5]
    assert F.region_areas(q4, status, 65535)[1].tolist() == [[5] * 5]
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            F.stereo_filter(q4, status, bad, 2)


def test_statuses_copied_and_bad_disparities_marked():
    q4 = np.array([[48, 48, 48, 48, 48, 0, -5, 65536, 65535, 1]], np.int32)
    status = np.array([[0, 1, 2, 3, 200, 0, 0, 0, 0, 0]], np.uint8)
    disp, st, depth, stats = F.stereo_filter(q4, status, 65535, 1, bf=2.0)
    assert st.tolist() == [[0, 1, 2, 3, 200, 3, 3, 3, 0, 0]]
    assert disp.tolist() == [[3.0, -1, -1, -1, -1, -1, -1, -1, 65535 / 16, 1 / 16]]
    assert stats.tolist() == [3, 0, 0, 3]
    # neither a copied status nor a marked pixel carries an edge: the two ends stay apart
    assert F.region_areas(q4, status, 65535)[1].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 2, 2]]
    assert F.stereo_filter(q4, status, 65535, 2)[1].tolist() == [[4, 1, 2, 3, 200, 3, 3, 3, 0, 0]]


def test_depth_bits():
    q4 = np.array([[1, 3, 7, 48, 65535, 100, 0]], np.int32); status = np.array([[0, 0, 0, 0, 0, 2, 0]], np.uint8)
    for bf in (75.0, 0.1, 1e-38, 3e38, 250.0):
        with np.errstate(over="ignore"):
            disp, st, depth, _ = F.stereo_filter(q4, status, 0, 1, bf=bf)
        bits = depth.view(np.uint32).tolist()[0]
        assert bits[5] == bits[6] == FLT_MAX_BITS
        for k in range(5):                                            # one correctly rounded fp32 division: the float64 quotient of two fp32 values rounded to fp32 is that value
            with np.errstate(over="ignore"):                          # (53 >= 2 x 24 + 2 bits: the second rounding of a quotient cannot change the result)
                want = np.float32(np.float64(np.float32(bf)) / np.float64(q4[0, k] / 16.0))
            assert bits[k] == struct.unpack("<I", struct.pack("<f", want))[0], (bf, k)
    assert struct.unpack("<I", struct.pack("<f", F.FLT_MAX))[0] == FLT_MAX_BITS and np.isfinite(F.FLT_MAX) and F.FLT_MAX > 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            F.stereo_filter(q4, status, 0, 1, bf=bad)


# ---- (e) the SGM statement's output ------------------------------------------------------------------
def test_on_sgm_output_removed_and_kept_regions_exist():
    name, q4, status, params, shows = CASES.sgm_case()
    assert params == dict(max_diff_q4=16, min_region=20) and shows(F)
    A, area = F.region_areas(q4, status, 16)
    roots = np.unique(A[A >= 0]); sizes = area.ravel()[roots]
    disp, st, _, stats = F.stereo_filter(q4, status, **params)
    print("valid %d, regions %d, below 20 px: %d regions with %d pixels" % (stats[0], len(roots), (sizes < 20).sum(), sizes[sizes < 20].sum()))
    assert stats[0] == (status == 0).sum() == sizes.sum()
    assert stats[1] == (sizes < 20).sum() > 0 and stats[2] == sizes[sizes < 20].sum() and (sizes >= 20).any()
    assert (stats[0], len(roots), stats[1], stats[2]) == (3339, 376, 335, 645)
    same((disp, st, None, stats), flood_fill(q4, status, 16, 20)[:4])


# ---- (f) the quality bar at the defaults -------------------------------------------------------------
def test_quality_bar_320x240_at_the_defaults():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import measure_stereo_filter as M
    from refimpl import stereo_sgm_np as G
    name, l, r, d, bf = M.pairs(1)[0]
    q4, status, right, wrong = M.populations(G, l, r, d, bf)
    assert int(right.sum() + wrong.sum()) == 73312 and int(wrong.sum()) == 339
    removed, lost = M.cell(F, q4, status, right, wrong, **F.DEFAULTS)
    print("defaults %s: wrong removed %.4f, right lost %.4f" % (F.DEFAULTS, removed, lost))
    assert lost <= 0.01 and removed > 0
    from vido_slam_amd import host
    assert (host.STEREO_FILTER_MAX_DIFF_Q4, host.STEREO_FILTER_MIN_REGION) == (F.DEFAULTS["max_diff_q4"], F.DEFAULTS["min_region"])
