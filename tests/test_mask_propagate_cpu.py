"""The label-image propagation rule (include/vido_c.h: vido_mask_propagate) on hand-made 8 x 8 cases: the numpy reference (tests/refimpl/mask_propagate_np.py) must give the
image worked out by hand for each.  The GPU tests compare the kernels with that reference bit for bit.  The built library must export the two entry points."""
import ctypes

import numpy as np
import pytest

from refimpl.mask_propagate_np import propagate, scatter_keys, EMPTY

H = W = 8


def maps(sources, depth=False):
    """sources: (x, y, label, dx, dy[, depth]) -> mask, flow (zeros elsewhere), depth (1.0 elsewhere) or None"""
    m = np.zeros((H, W), np.int32); f = np.zeros((H, W, 2), np.float32); d = np.ones((H, W), np.float32)
    for s in sources:
        x, y, lab, dx, dy = s[:5]
        m[y, x] = lab; f[y, x] = (dx, dy)
        if len(s) > 5:
            d[y, x] = s[5]
    return m, f, (d if depth else None)


def image(pixels):
    out = np.zeros((H, W), np.int32)
    for (x, y), lab in pixels.items():
        out[y, x] = lab
    return out


def check(sources, pixels, stats, depth=False):
    m, f, d = maps(sources, depth)
    m0 = m.copy()
    out, st = propagate(m, f, d)
    assert out.dtype == np.int32 and st.dtype == np.int32
    assert np.array_equal(out, image(pixels)), (out, image(pixels))
    assert st.tolist() == list(stats), st
    assert np.array_equal(m, m0)


def test_nearer_source_wins_and_without_depth_the_smaller_label():
    src = [(1, 1, 3, 2, 0, 2.0), (5, 1, 9, -2, 0, 1.0)]                # both land on (3, 1); label 9 is nearer
    check(src, {(3, 1): 9}, (2, 1, 0), depth=True)
    check(src, {(3, 1): 3}, (2, 1, 0), depth=False)
    # the key itself: depth bits above the label
    plane, n = scatter_keys(*maps(src, True))
    assert n == 2 and int(plane[1, 3]) == (int(np.float32(1.0).view(np.uint32)) << 32 | 9) and (plane != EMPTY).sum() == 1


def test_equal_depth_smaller_label_wins():
    check([(1, 1, 9, 2, 0, 2.0), (5, 1, 3, -2, 0, 2.0)], {(3, 1): 3}, (2, 1, 0), depth=True)
    check([(1, 1, 3, 2, 0, 2.0), (5, 1, 9, -2, 0, 2.0)], {(3, 1): 3}, (2, 1, 0), depth=True)


def test_five_votes_fill_a_hole_four_do_not_and_nothing_cascades():
    five = [(2, 2), (3, 2), (4, 2), (2, 3), (4, 3)]                    # 5 of the 8 neighbours of (3, 3)
    check([(x, y, 7, 0, 0) for x, y in five], {**{p: 7 for p in five}, (3, 3): 7}, (5, 5, 1))
    four = five[:-1]
    check([(x, y, 7, 0, 0) for x, y in four], {p: 7 for p in four}, (4, 4, 0))
    # all 8: filled as well
    ring = [(x, y) for y in (2, 3, 4) for x in (2, 3, 4) if (x, y) != (3, 3)]
    check([(x, y, 7, 0, 0) for x, y in ring], {**{p: 7 for p in ring}, (3, 3): 7}, (8, 8, 1))
    # one pass: (3, 3) has 5 votes; (4, 3) has 4 and would have 5 if (3, 3)'s fill counted
    hits = [(2, 2), (3, 2), (4, 2), (2, 3), (2, 4), (5, 2), (5, 3)]
    check([(x, y, 7, 0, 0) for x, y in hits], {**{p: 7 for p in hits}, (3, 3): 7}, (7, 7, 1))


def test_hole_next_to_two_labels():
    ring = [(2, 2), (3, 2), (4, 2), (2, 3), (4, 3), (2, 4), (3, 4), (4, 4)]
    half = {p: (2 if i < 4 else 3) for i, p in enumerate(ring)}        # 4 + 4: no label has 5
    check([(x, y, lab, 0, 0) for (x, y), lab in half.items()], half, (8, 8, 0))
    most = {p: (2 if i < 5 else 3) for i, p in enumerate(ring)}        # 5 + 3: label 2
    check([(x, y, lab, 0, 0) for (x, y), lab in most.items()], {**most, (3, 3): 2}, (8, 8, 1))
    # 5 neighbours hit, but by 3 + 2 of two labels: nothing
    mixed = {(2, 2): 2, (3, 2): 2, (4, 2): 2, (2, 3): 3, (4, 3): 3}
    check([(x, y, lab, 0, 0) for (x, y), lab in mixed.items()], mixed, (5, 5, 0))


def test_half_integers_round_to_even():
    # one source per row, from x = 3: 0.5 -> 0, 1.5 -> 2, -0.5 -> 0, 2.5 -> 2, -1.5 -> -2, -2.5 -> -2; and in y on the last rows
    src = [(3, 0, 1, 0.5, 0), (3, 1, 2, 1.5, 0), (3, 2, 3, -0.5, 0), (3, 3, 4, 2.5, 0), (3, 4, 5, -1.5, 0), (3, 5, 6, -2.5, 0), (0, 6, 7, 0, 0.5), (1, 6, 8, 0, -1.5)]
    out, st = propagate(*maps(src))
    assert np.array_equal(out, image({(3, 0): 1, (5, 1): 2, (3, 2): 3, (5, 3): 4, (1, 5): 6, (0, 6): 7, (1, 4): 5}))      # (1, 6) -> (1, 4) collides with label 5 there: 5 < 8
    assert st.tolist() == [8, 7, 0]


def test_targets_on_and_just_past_each_border():
    on = [(1, 3, 1, -1, 0), (6, 3, 2, 1, 0), (3, 1, 3, 0, -1), (3, 6, 4, 0, 1), (0, 5, 5, -0.5, 0), (7, 5, 6, 0.5, 0)]       # -0.5 / 0.5 round to 0: still inside
    check(on, {(0, 3): 1, (7, 3): 2, (3, 0): 3, (3, 7): 4, (0, 5): 5, (7, 5): 6}, (6, 6, 0))
    past = [(1, 3, 1, -2, 0), (6, 3, 2, 2, 0), (3, 1, 3, 0, -2), (3, 6, 4, 0, 2), (0, 5, 5, -0.51, 0), (7, 5, 6, 0.51, 0), (7, 7, 7, 1, 1), (0, 0, 8, -1, -1)]
    check(past, {}, (0, 0, 0))


def test_hostile_flow_and_unusable_depth_are_skipped():
    bad_flow = [(1, 1, 1, np.nan, 0), (2, 1, 1, 0, np.nan), (3, 1, 1, np.inf, 0), (4, 1, 1, 0, -np.inf), (5, 1, 1, 1e30, 0), (6, 1, 1, 0, -1e30), (1, 2, 1, 32768.0, 0),
                (2, 2, 1, -32768.0, 0), (3, 2, 1, 32767.0, 0)]         # the last one is a source, but its target is far outside
    check(bad_flow + [(4, 4, 2, 0, 0)], {(4, 4): 2}, (1, 1, 0))
    bad_depth = [(1, 1, 1, 0, 0, 0.0), (2, 1, 1, 0, 0, -1.0), (3, 1, 1, 0, 0, np.nan), (4, 1, 1, 0, 0, np.inf), (5, 1, 1, 0, 0, -0.0), (6, 1, 1, 0, 0, -np.inf)]
    check(bad_depth + [(4, 4, 2, 0, 0, 3.5)], {(4, 4): 2}, (1, 1, 0), depth=True)
    # without a depth map the same pixels all scatter
    check(bad_depth, {(x, 1): 1 for x in range(1, 7)}, (6, 6, 0), depth=False)


def test_labels_not_above_zero_never_scatter():
    check([(1, 1, 0, 1, 0), (2, 2, -3, 1, 0), (3, 3, -2147483648, 0, 0), (4, 4, 70000, 1, 1), (5, 1, 2147483647, 0, 0)], {(5, 5): 70000, (5, 1): 2147483647}, (2, 2, 0))
    # a ring of negative labels around a hole fills nothing
    ring = [(x, y) for y in (2, 3, 4) for x in (2, 3, 4) if (x, y) != (3, 3)]
    check([(x, y, -7, 0, 0) for x, y in ring], {}, (0, 0, 0))


def test_all_zero_and_single_label_images():
    z = np.zeros((H, W), np.int32); f = np.ones((H, W, 2), np.float32)
    out, st = propagate(z, f)
    assert not out.any() and st.tolist() == [0, 0, 0]
    one = np.full((H, W), 4, np.int32)
    out, st = propagate(one, f, np.ones((H, W), np.float32))           # everything moves by (1, 1): row 0 and column 0 are vacated; (0, 0) .. have < 5 hit neighbours
    exp = np.zeros((H, W), np.int32); exp[1:, 1:] = 4
    assert np.array_equal(out, exp) and st.tolist() == [49, 49, 0]


def test_library_exports_the_entry_points(vido):
    lib = ctypes.CDLL(vido.LIB_PATH)
    for name in ("vido_mask_propagate", "vido_frame_propagate_mask"):
        assert hasattr(lib, name), name
