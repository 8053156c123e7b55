"""The numpy statement of vido_mask_components (tests/refimpl/mask_components_np.py) itself: hand-made cases whose answer is written out, scipy.ndimage.label as an
independent labeller on the seeded images the GPU test uses, and the convoy's class image (five cars, one class) splitting into its five objects.  No GPU."""
import numpy as np
import pytest

from refimpl import cc_patterns as P
from refimpl.mask_components_np import anchors, components


def test_two_values_touching_never_join():
    m = np.array([[3, 3, 7, 7],
                  [3, 3, 7, 7],
                  [0, 0, 7, 3]], np.int32)
    out, classes, areas, stats = components(m, 8)
    assert out.tolist() == [[1, 1, 2, 2], [1, 1, 2, 2], [0, 0, 2, 3]]
    assert classes[:4].tolist() == [3, 7, 3, 0] and areas[:4].tolist() == [4, 5, 1, 0] and stats.tolist() == [3, 0, 0, 3]
    assert out.dtype == np.int32 and classes.dtype == np.int64 and areas.dtype == np.int32 and classes.shape == (127,)


def test_a_diagonal_pair_under_both_connectivities():
    m = np.array([[5, 0],
                  [0, 5]], np.int32)
    assert components(m, 8)[0].tolist() == [[1, 0], [0, 1]] and components(m, 8)[3].tolist() == [1, 0, 0, 1]
    assert components(m, 4)[0].tolist() == [[1, 0], [0, 2]] and components(m, 4)[3].tolist() == [2, 0, 0, 2]
    m = np.array([[0, 5],
                  [5, 0]], np.int32)                                  # the other diagonal: the anchor is the upper right pixel
    assert components(m, 8)[0].tolist() == [[0, 1], [1, 0]]
    assert components(m, 4)[0].tolist() == [[0, 1], [2, 0]]
    assert anchors(m, 8).tolist() == [[-1, 1], [1, -1]]


def test_min_area_drops_before_the_ranks_are_given():
    m = np.array([[2, 0, 2, 2, 0, 2],
                  [0, 0, 2, 0, 0, 2],
                  [2, 2, 0, 0, 0, 2]], np.int32)
    out, classes, areas, stats = components(m, 4, min_area=3)
    assert out.tolist() == [[0, 0, 1, 1, 0, 2], [0, 0, 1, 0, 0, 2], [0, 0, 0, 0, 0, 2]]
    assert areas[:3].tolist() == [3, 3, 0] and stats.tolist() == [4, 2, 0, 2]
    for ma in (1, 0, -5):                                             # min_area <= 1 keeps all
        out, _, areas, stats = components(m, 4, min_area=ma)
        assert out.tolist() == [[1, 0, 2, 2, 0, 3], [0, 0, 2, 0, 0, 3], [4, 4, 0, 0, 0, 3]] and stats.tolist() == [4, 0, 0, 4]
    assert components(m, 4, min_area=4)[3].tolist() == [4, 4, 0, 0]


def test_the_cap_cuts_in_anchor_order_and_the_id_base_shifts():
    m = P.checkerboard(4, 6)                                          # 12 single pixels under 4-connectivity
    out, classes, areas, stats = components(m, 4, cap=5, id_base=127)
    assert stats.tolist() == [12, 0, 7, 5]
    assert out.ravel()[np.flatnonzero(m.ravel())].tolist() == [128, 129, 130, 131, 132, 0, 0, 0, 0, 0, 0, 0]
    assert classes.tolist() == [5] * 5 and areas.tolist() == [1] * 5
    assert components(m, 8, cap=5)[3].tolist() == [1, 0, 0, 1]
    # dropped components do not use up the cap: two big ones behind three single pixels
    m = np.zeros((4, 12), np.int32); m[0, 0] = m[0, 2] = m[0, 4] = 1; m[2:, 0:3] = 1; m[2:, 6:9] = 1
    out, _, areas, stats = components(m, 8, min_area=2, cap=2)
    assert stats.tolist() == [5, 3, 0, 2] and areas.tolist() == [6, 6] and out[3, 0] == 1 and out[3, 6] == 2 and out[0].sum() == 0


def test_hostile_values():
    big, low = 2147483647, -2147483648
    m = np.array([[big, big, 0, -1, low],
                  [big - 1, big, -1, -1, low],
                  [1, 255, 256, 65536, 65536]], np.int32)
    out, classes, areas, stats = components(m, 8)
    assert out.tolist() == [[1, 1, 0, 0, 0], [2, 1, 0, 0, 0], [3, 4, 5, 6, 6]]
    assert classes[:7].tolist() == [big, big - 1, 1, 255, 256, 65536, 0] and areas[:6].tolist() == [3, 1, 1, 1, 1, 2] and stats.tolist() == [6, 0, 0, 6]


def test_the_patterns_are_what_their_names_say():
    for H, W in ((64, 64), (201, 151)):
        assert components(P.spirals(H, W), 8)[3].tolist() == [2, 0, 0, 2] and components(P.spirals(H, W), 4)[3].tolist() == [2, 0, 0, 2]
        assert (P.spirals(H, W) == 11).sum() > 3 * min(H, W) and (P.spirals(H, W) == 12).sum() > 3 * min(H, W)
        for pat in (P.serpentine, P.comb, P.full):
            for conn in (4, 8):
                out, _, areas, stats = components(pat(H, W), conn)
                assert stats.tolist() == [1, 0, 0, 1] and areas[0] == (pat(H, W) > 0).sum() and np.array_equal(out > 0, pat(H, W) > 0)
        for anti in (False, True):
            assert components(P.corner_touch(H, W, anti), 8)[3][0] == 1 and components(P.corner_touch(H, W, anti), 4)[3][0] == 2
        assert components(P.checkerboard(H, W), 8)[3].tolist() == [1, 0, 0, 1]
        assert components(P.checkerboard(H, W), 4)[3].tolist() == [(H * W + 1) // 2, 0, (H * W + 1) // 2 - 127, 127]
        assert components(P.empty(H, W), 8)[3].tolist() == [0, 0, 0, 0] and not components(P.empty(H, W), 8)[0].any()
    for H, W in ((1, 777), (777, 1)):
        for pat in (P.spirals, P.serpentine, P.comb, P.full, P.checkerboard, P.corner_touch, P.empty):
            components(pat(H, W), 8)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("H,W", ((64, 64), (201, 151), (375, 1242), (1, 777), (777, 1)))
def test_equals_scipy_label_per_value_merged_by_anchor(H, W, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    m = P.blobs(H, W, 31 + H + W)
    structure = np.ones((3, 3), int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    comps = []                                                        # (anchor, value, area, pixel mask) of every component, value by value
    for v in np.unique(m[m > 0]):
        lab, n = ndi.label(m == v, structure=structure)
        flat = lab.ravel()
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        cnt = np.bincount(flat, minlength=n + 1)
        comps += [(int(first[k]), int(v), int(cnt[k]), k, lab) for k in range(1, n + 1)]
    comps.sort(key=lambda c: c[0])
    for min_area in (1, 20):
        surv = [c for c in comps if c[2] >= min_area]
        want = np.zeros((H, W), np.int32)
        for k, (_, v, a, lk, lab) in enumerate(surv[:127]):
            want[lab == lk] = 1 + k
        out, classes, areas, stats = components(m, conn, min_area=min_area)
        kept = min(len(surv), 127)
        assert stats.tolist() == [len(comps), len(comps) - len(surv), len(surv) - kept, kept]
        assert np.array_equal(out, want)
        assert classes[:kept].tolist() == [c[1] for c in surv[:kept]] and areas[:kept].tolist() == [c[2] for c in surv[:kept]]
        assert not classes[kept:].any() and not areas[kept:].any()
    assert len(comps) > 5


def test_the_convoys_class_image_splits_into_its_five_cars():
    from vido_slam_amd import synth
    scene = synth.convoy_scene(9)
    for k in range(8):
        gt = scene.frame(k)[3]
        out, classes, areas, stats = components((3 * (gt > 0)).astype(np.int32), 8)
        assert stats.tolist() == [5, 0, 0, 5] and classes[:6].tolist() == [3, 3, 3, 3, 3, 0]
        for i in range(1, 6):                                         # each component is one ground-truth object
            ids = np.unique(out[gt == i])
            assert len(ids) == 1 and ids[0] > 0 and (out == ids[0]).sum() == (gt == i).sum() == areas[ids[0] - 1]
