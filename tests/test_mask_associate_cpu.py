"""The overlap association rule (include/vido_c.h: vido_mask_associate) on hand-made 8 x 8 and 16 x 16 cases: the numpy reference (tests/refimpl/mask_associate_np.py) must
give the answer worked out by hand for each.  The GPU tests compare the kernels with that reference bit for bit.  The header must declare the entry point and the built
library export it."""
import ctypes
import os

import numpy as np

from refimpl.mask_associate_np import associate, clean, STATE_WORDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def image(H, W, rects):
    """rects: (value, y0, y1, x0, x1), half-open, later ones on top"""
    m = np.zeros((H, W), np.int32)
    for v, y0, y1, x0, x1 in rects:
        m[y0:y1, x0:x1] = v
    return m


def fresh_state(cursor=0, classes=None, lost=None):
    s = np.zeros(STATE_WORDS, np.int32)
    s[0] = cursor
    for i, c in (classes or {}).items():
        s[256 + i] = c
    for i, l in (lost or {}).items():
        s[512 + i] = l
    return s


def cls(*v):
    return np.array(v, np.int64)


def test_an_instance_takes_over_the_id_it_overlaps():
    prev = image(8, 8, [(7, 1, 4, 1, 5)])                             # 12 pixels
    cur = image(8, 8, [(1, 1, 4, 2, 6)])                              # 12 pixels, 9 shared: IoU 9 / 15
    st0 = fresh_state(cursor=7, classes={7: 3})
    out, lut, st, stats = associate(prev, cur, 1, cls(5), 0, st0)
    assert np.array_equal(out, image(8, 8, [(7, 1, 4, 2, 6)]))        # the detector's footprint under the old id; the column only prev covered is background
    assert lut[1] == 7 and not lut[2:].any() and lut[0] == 0
    assert stats.tolist() == [1, 0, 0, 0]
    assert st[0] == 7 and st[256 + 7] == 5 and st[512 + 7] == 0       # the class is the detector's of THIS frame
    assert np.array_equal(st0, fresh_state(cursor=7, classes={7: 3})) # the input state is not modified
    assert out.dtype == np.int32 and lut.dtype == np.int32 and st.dtype == np.int32 and stats.dtype == np.int32


def test_iou_of_exactly_one_half_is_no_match_and_one_more_shared_pixel_is():
    prev = image(8, 8, [(5, 2, 3, 0, 6)])                             # Ap = 6
    cur = image(8, 8, [(1, 2, 3, 2, 8)])                              # Ac = 6, C = 4: IoU 4 / 8
    out, lut, st, stats = associate(prev, cur, 1, None, 0, fresh_state())
    assert lut[1] == 1 and stats.tolist() == [0, 1, 1, 0]             # a fresh id (the cursor's next), the old one lost and, with hold = 0, retired
    assert np.array_equal(out, image(8, 8, [(1, 2, 3, 2, 8)]))
    assert st[0] == 1 and st[256 + 1] == 1 and st[256 + 5] == 0
    cur = image(8, 8, [(1, 2, 3, 1, 7)])                              # Ac = 6, C = 5: IoU 5 / 7
    out, lut, st, stats = associate(prev, cur, 1, None, 0, fresh_state())
    assert lut[1] == 5 and stats.tolist() == [1, 0, 0, 0]
    assert np.array_equal(out, image(8, 8, [(5, 2, 3, 1, 7)])) and st[0] == 0


def test_fresh_ids_skip_the_ids_of_the_previous_image():
    prev = image(8, 8, [(1, 0, 1, 0, 2), (2, 0, 1, 3, 5), (4, 0, 1, 6, 8)])
    cur = image(8, 8, [(1, 4, 6, 0, 3), (2, 4, 6, 4, 8)])
    out, lut, st, stats = associate(prev, cur, 2, cls(3, 3), 0, fresh_state())
    assert lut[1] == 3 and lut[2] == 5                                # 1, 2 and 4 are in the previous image
    assert stats.tolist() == [0, 2, 3, 0] and st[0] == 5
    assert np.array_equal(out, image(8, 8, [(3, 4, 6, 0, 3), (5, 4, 6, 4, 8)]))
    assert [int(st[256 + i]) for i in range(1, 7)] == [0, 0, 3, 0, 3, 0]


def test_the_cursor_wraps_from_254_to_1():
    cur = image(8, 8, [(1, 0, 2, 0, 2), (2, 0, 2, 3, 5), (3, 4, 6, 0, 2)])
    out, lut, st, stats = associate(None, cur, 3, None, 0, fresh_state(cursor=253))
    assert lut[1:4].tolist() == [254, 1, 2] and st[0] == 2 and stats.tolist() == [0, 3, 0, 0]
    assert np.array_equal(out, image(8, 8, [(254, 0, 2, 0, 2), (1, 0, 2, 3, 5), (2, 4, 6, 0, 2)]))
    # a cursor outside 0..254 reads as 0
    assert associate(None, cur, 3, None, 0, fresh_state(cursor=-5))[1][1:4].tolist() == [1, 2, 3]
    assert associate(None, cur, 3, None, 0, fresh_state(cursor=255))[1][1:4].tolist() == [1, 2, 3]


def test_a_retired_id_is_not_handed_out_on_the_next_frame():
    prev = image(8, 8, [(9, 2, 5, 2, 5)])
    st0 = fresh_state(cursor=9, classes={9: 3})
    out, lut, st1, stats = associate(prev, np.zeros((8, 8), np.int32), 0, cls(), 0, st0)
    assert not out.any() and stats.tolist() == [0, 0, 1, 0]
    assert st1[256 + 9] == 0 and st1[512 + 9] == 0 and st1[0] == 9    # retired; the cursor stays behind it
    cur = image(8, 8, [(1, 2, 5, 2, 5)])                              # the same place, a frame later: nothing of 9 is left to match
    out, lut, st2, stats = associate(out, cur, 1, cls(3), 0, st1)
    assert lut[1] == 10 and st2[0] == 10 and stats.tolist() == [0, 1, 0, 0]
    assert np.array_equal(out, image(8, 8, [(10, 2, 5, 2, 5)]))


def test_hostile_labels_count_as_background():
    cur = image(8, 8, [(1, 0, 2, 0, 4), (2, 2, 4, 0, 4), (3, 4, 6, 0, 4), (-4, 6, 8, 0, 4), (2147483647, 0, 8, 6, 8)])
    prev = image(8, 8, [(255, 0, 2, 0, 4), (-3, 4, 6, 0, 4), (300, 6, 8, 0, 4), (-2147483648, 0, 8, 6, 8)])
    classes = cls(0, 3)                                               # slot 0 is an unused slot; value 3 is past n = 2
    p, c = clean(prev, cur, 2, classes)
    assert not p.any() and set(np.unique(c).tolist()) == {0, 2}
    out, lut, st, stats = associate(prev, cur, 2, classes, 5, fresh_state())
    assert np.array_equal(out, image(8, 8, [(1, 2, 4, 0, 4)]))        # slot 1 alone, under the first id; nothing of prev is held although hold = 5
    assert lut[2] == 1 and lut[1] == 0 and lut[3] == 0 and stats.tolist() == [0, 1, 0, 0]
    assert st[256 + 1] == 3 and not st[257 + 1:512].any()


def run_miss(hold):
    """Detected on frame 0, missed on frames 1-4 (the warp is the identity), detected again on frame 5 -> per frame (ids in the image, stats), and the last state."""
    box = image(8, 8, [(1, 2, 6, 2, 6)]); none = np.zeros((8, 8), np.int32)
    st = fresh_state(); prev = None; seen = []
    for k in range(6):
        det = k in (0, 5)
        prev, lut, st, stats = associate(prev, box if det else none, 1 if det else 0, cls(3) if det else cls(), hold, st)
        seen.append((sorted(set(np.unique(prev).tolist()) - {0}), stats.tolist()))
    return seen, st


def test_hold_through_a_four_frame_miss():
    seen, st = run_miss(0)
    assert seen == [([1], [0, 1, 0, 0]), ([], [0, 0, 1, 0]), ([], [0, 0, 0, 0]), ([], [0, 0, 0, 0]), ([], [0, 0, 0, 0]), ([2], [0, 1, 0, 0])]
    seen, st = run_miss(1)
    assert seen == [([1], [0, 1, 0, 0]), ([1], [0, 0, 1, 0]), ([], [0, 0, 1, 0]), ([], [0, 0, 0, 0]), ([], [0, 0, 0, 0]), ([2], [0, 1, 0, 0])]
    assert st[256 + 1] == 0 and st[256 + 2] == 3
    seen, st = run_miss(2)
    assert seen == [([1], [0, 1, 0, 0]), ([1], [0, 0, 1, 0]), ([1], [0, 0, 1, 0]), ([], [0, 0, 1, 0]), ([], [0, 0, 0, 0]), ([2], [0, 1, 0, 0])]
    # a hold that outlasts the miss: the object is in the image throughout and gets its old id back
    seen, st = run_miss(4)
    assert [s[0] for s in seen] == [[1]] * 6 and seen[5][1] == [1, 0, 0, 0] and seen[4][1] == [0, 0, 1, 0]
    assert st[0] == 1 and st[256 + 1] == 3 and st[512 + 1] == 0


def test_a_held_id_keeps_its_class_and_counts_its_lost_frames():
    prev = image(8, 8, [(6, 1, 3, 1, 3)])
    out, lut, st, stats = associate(prev, np.zeros((8, 8), np.int32), 0, None, 3, fresh_state(cursor=6, classes={6: 8}, lost={6: 1}))
    assert np.array_equal(out, prev) and st[256 + 6] == 8 and st[512 + 6] == 2 and stats.tolist() == [0, 0, 1, 0]
    # an id the state knows but the warped image has lost entirely (it left the frame) is cleared at once, whatever the hold
    out, lut, st, stats = associate(None, np.zeros((8, 8), np.int32), 0, None, 3, fresh_state(cursor=6, classes={6: 8}, lost={6: 1}))
    assert st[256 + 6] == 0 and st[512 + 6] == 0 and stats.tolist() == [0, 0, 0, 0]


def test_no_free_id_leaves_the_instance_out():
    prev = np.zeros(256, np.int32); prev[:254] = np.arange(1, 255)    # 254 ids, a pixel each
    prev = prev.reshape(16, 16)
    cur = np.zeros((16, 16), np.int32); cur[15, 14:] = 1
    out, lut, st, stats = associate(prev, cur, 1, cls(3), 0, fresh_state(cursor=17))
    assert lut[1] == 0 and stats.tolist() == [0, 0, 254, 1] and stats[3] == 1
    assert not out.any() and st[0] == 17 and not st[256:].any()
    # with a hold the 254 stay, and the instance is still left out
    out, lut, st, stats = associate(prev, cur, 1, cls(3), 1, fresh_state(cursor=17))
    assert np.array_equal(out, prev) and stats.tolist() == [0, 0, 254, 1] and (st[513:767] == 1).all()
    # one id fewer in the image: that id is the only free one, wherever the cursor stands
    prev2 = prev.copy(); prev2[prev2 == 100] = 0
    out, lut, st, stats = associate(prev2, cur, 1, cls(3), 0, fresh_state(cursor=200))
    assert lut[1] == 100 and st[0] == 100 and stats.tolist() == [0, 1, 253, 0]


def test_header_declares_and_library_exports_the_entry_point(vido):
    txt = open(os.path.join(ROOT, "include", "vido_c.h")).read()
    assert "int vido_mask_associate(vido_ctx* ctx" in txt
    lib = ctypes.CDLL(vido.LIB_PATH)
    assert hasattr(lib, "vido_mask_associate")
