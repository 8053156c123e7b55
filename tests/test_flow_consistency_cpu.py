"""CPU: the statement of vido_flow_consistency (tests/refimpl/flow_consistency_np.py) — the numpy form against the same rule written per pixel in Python integers on
constructed fields at 5 x 4, 16 x 16 and 4095 x 1 (tests/refimpl/flow_consistency_cases.py), what follows from the definition alone, the bounds its docstring states, and
that every status occurs on the translation pairs of tests/test_dis_flow_gpu.py.  The kernel is bound to the statement by equality (tests/test_flow_consistency_gpu.py)."""
import numpy as np
import pytest

from refimpl import dis_flow_np as D
from refimpl import flow_consistency_np as F
from refimpl import flow_consistency_cases as K


def _well_formed(fwd, status, marked, stats):
    h, w = fwd.shape[:2]
    assert status.dtype == np.uint8 and status.shape == (h, w) and marked.dtype == np.float32 and marked.shape == (h, w, 2) and stats.dtype == np.int32 and stats.shape == (4,)
    assert stats.sum() == h * w and [int((status == k).sum()) for k in range(4)] == stats.tolist()
    bits = marked.view(np.uint32)
    assert (bits[status != 0] == F.NAN_BITS).all()                                           # the stated NaN, on both components, exactly where the status is not 0
    assert np.array_equal(bits[status == 0], (fwd[status == 0].astype(np.float32) / np.float32(256)).view(np.uint32))
    assert not np.isnan(marked[status == 0]).any()


@pytest.mark.parametrize("case", K.constructed(), ids=lambda c: c[0])
def test_statement_equals_the_rule_per_pixel_in_python_integers(case):
    name, fwd, bwd, alpha, beta = case
    terms = []
    status, marked, stats = F.flow_consistency(fwd, bwd, alpha, beta)
    assert np.array_equal(status, K.by_pixels(fwd, bwd, alpha, beta, terms)), name
    _well_formed(fwd, status, marked, stats)
    assert max(terms) < 1 << 52                                                               # every term of the decision, with room in int64
    print("%-24s stats %s, largest term 2^%.1f" % (name, stats.tolist(), np.log2(max(max(terms), 1))))


@pytest.mark.parametrize("h,w", [(4, 5), (16, 16)])
def test_targets_on_and_past_the_border(h, w):
    (name, fwd, bwd, alpha, beta), want = K.borders(h, w)
    status = F.flow_consistency(fwd, bwd, alpha, beta)[0]
    assert np.array_equal(status, want)
    assert status[0, w - 2] == 0 and status[h - 2, 1] == 0 and status[h - 1, w - 1] == 0      # exactly on 256 (W - 1) / 256 (H - 1) is in
    assert status[1, w - 2] == 2 and status[h - 2, 2] == 2 and status[2, 0] == 2 and status[0, 2] == 2


@pytest.mark.parametrize("h,w", [(4, 5), (16, 16)])
def test_clamped_neighbours_and_the_largest_fractions(h, w):
    name, fwd, bwd, alpha, beta = K.clamps_and_fractions(h, w, 3 + w)
    b, st = F.backward_at_target(fwd, bwd)
    B = bwd.astype(np.int64)
    assert st[1, w - 2] == 0 and np.array_equal(b[1, w - 2], B[1, w - 1])                    # ax = 0 on the last column: x1 clamps, the tap itself
    assert st[h - 2, 1] == 0 and np.array_equal(b[h - 2, 1], B[h - 1, 1])
    assert np.array_equal(b[h - 2, w - 2], B[h - 1, w - 1]) and np.array_equal(b[h - 1, w - 1], B[h - 1, w - 1])
    assert np.array_equal(b[h - 1, w - 2], (56 * B[h - 1, w - 2] + 200 * B[h - 1, w - 1] + 128) >> 8)      # last row: y1 = y0, the weights of both rows on one
    assert np.array_equal(b[h - 2, w - 1], (56 * B[h - 2, w - 1] + 200 * B[h - 1, w - 1] + 128) >> 8)
    want = (1 * B[1, 1] + 255 * B[1, 2] + 255 * B[2, 1] + 65025 * B[2, 2] + 32768) >> 16                   # ax = ay = 255
    assert np.array_equal(b[1, 1], want)
    for y in range(h):
        for x in range(w):
            status, b_px = K.pixel(fwd, bwd, x, y, alpha, beta)
            if b_px is None:
                assert st[y, x] == status
            else:
                assert st[y, x] == 0 and b_px == b[y, x].tolist()


@pytest.mark.parametrize("h,w", [(4, 5), (16, 16)])
def test_rounding_of_negative_sums(h, w):
    (name, fwd, bwd, alpha, beta), pixels, want = K.negative_rounding(h, w)
    b, st = F.backward_at_target(fwd, bwd)
    assert [int(b[y, x, 0]) for x, y in pixels] == list(want) and all(st[y, x] == 0 for x, y in pixels)
    assert (-32768 + 32768) >> 16 == 0 and (-98304 + 32768) >> 16 == -1 and (-65536 + 32768) >> 16 == -1 and (-32769 + 32768) >> 16 == -1


def test_extremes_stay_inside_int64_and_the_limit_is_not_a_flow():
    for h, w in ((4, 5), (16, 16)):
        name, fwd, bwd, alpha, beta = K.extremes(h, w)
        assert alpha == 1024 and beta == 1 << 30
        status = F.flow_consistency(fwd, bwd, alpha, beta)[0]
        assert status[0, 0] in (0, 1) and status[1, 1] in (0, 1)                              # taps of +-(2^19 - 1) are flows
        assert status[2, 2] == 2 and status[1, 3] == 2 and status[1, 2] == 2                  # a forward +-(2^19 - 1) is a flow that leaves a small image
        assert (status[3, :3] == 3).all() and status[2, 0] == 3 and status[2, 1] == 3         # +-2^19 and the int32 extremes are none
        assert status[h - 1, w - 2] == 3 and status[h - 2, w - 1] == 3 and status[h - 1, w - 1] == 3      # a single tap at 2^19, through three different tap positions
        assert status[h - 2, w - 2] == 3                                                       # ... and as the tap of weight 0 of the pixel that rests diagonally before it
        assert status[h - 3, w - 1] == 0                                                       # a pixel none of whose taps it is
    name, fwd, bwd, alpha, beta = K.widest()
    terms = []
    status = F.flow_consistency(fwd, bwd, alpha, beta)[0]
    assert np.array_equal(status, K.by_pixels(fwd, bwd, alpha, beta, terms))
    T = K.TOP
    worst_lhs = 1024 * ((2 * T) ** 2 + T ** 2)                                                # r = (2 (2^19 - 1), 2^19 - 1): reached at pixel 0
    assert max(terms) >= worst_lhs and max(terms) < 1 << 52
    assert 1024 * 2 * (2 * T + 1) ** 2 < 1 << 52 and 1024 * 4 * T * T + 1024 * (1 << 30) < 1 << 52      # the bounds of the docstring, in Python integers
    assert status[0, 0] == 1 and status[0, 4095 - 81] == 1 and status[0, 40] == 0 and status[0, 4095 - 121] == 0


@pytest.mark.parametrize("h,w", [(4, 5), (16, 16)])
def test_alpha_and_beta_zero_pass_only_r_zero(h, w):
    name, fwd, bwd, alpha, beta = K.exact_only(h, w)
    assert alpha == 0 and beta == 0
    status, marked, stats = F.flow_consistency(fwd, bwd, alpha, beta)
    want = np.zeros((h, w), np.uint8); want[:, w - 1] = 2; want[1, 1] = 1
    assert np.array_equal(status, want)
    assert F.flow_consistency(fwd, bwd, 0, 1)[0][1, 1] == 0                                   # |r|^2 = (1/256 px)^2 = 2^-16 px^2 = beta_q16 1: equality passes
    _well_formed(fwd, status, marked, stats)


@pytest.mark.parametrize("dx,dy", [(1, 0), (-3, 2), (0, -5), (7, 7)])
def test_an_integer_translation_and_its_negation_is_consistent_everywhere_inside(dx, dy):
    for h, w in ((4, 5), (16, 16), (50, 73)):
        fwd, bwd = K.translation(h, w, dx, dy)
        status, marked, stats = F.flow_consistency(fwd, bwd, 0, 0)
        Y, X = np.mgrid[0:h, 0:w]
        inside = (X + dx >= 0) & (X + dx <= w - 1) & (Y + dy >= 0) & (Y + dy <= h - 1)
        assert np.array_equal(status, np.where(inside, 0, 2))
        assert np.array_equal(F.flow_consistency(fwd, bwd)[0], status)
        _well_formed(fwd, status, marked, stats)


def test_parameter_limits():
    f = np.zeros((4, 5, 2), np.int32)
    for kw in (dict(alpha_q10=-1), dict(alpha_q10=1025), dict(beta_q16=-1), dict(beta_q16=(1 << 30) + 1)):
        with pytest.raises(ValueError):
            F.flow_consistency(f, f, **kw)
    assert F.flow_consistency(np.zeros((1, 1, 2), np.int32), np.zeros((1, 1, 2), np.int32))[2].tolist() == [1, 0, 0, 0]
    assert F.DEFAULTS == dict(alpha_q10=10, beta_q16=32768)


@pytest.mark.parametrize("w,h,coarsest", [(64, 64, 2), (73, 50, 2), (201, 151, 3)])
def test_every_status_occurs_on_the_translation_pairs(vido, w, h, coarsest):
    """Not vacuous: on the sub-pixel translation pairs of tests/test_dis_flow_gpu.py the statement's two flows give consistent, inconsistent and leaving pixels at the
    defaults."""
    from test_dis_flow_gpu import _pair
    a, b = _pair(vido, w, h, seed=w + coarsest)
    fwd, bwd = D.dis_flow(a, b, coarsest=coarsest)[1], D.dis_flow(b, a, coarsest=coarsest)[1]
    status, marked, stats = F.flow_consistency(fwd, bwd)
    print("%d x %d: stats %s" % (w, h, stats.tolist()))
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] == 0
    assert stats[0] > stats[1] + stats[2]                                                     # ... and most of a translated image is consistent
    _well_formed(fwd, status, marked, stats)


def test_at_16_x_16_an_inconsistent_pixel_needs_the_tightest_rule(vido):
    from test_dis_flow_gpu import _pair
    a, b = _pair(vido, 16, 16, seed=17)
    fwd, bwd = D.dis_flow(a, b, coarsest=1)[1], D.dis_flow(b, a, coarsest=1)[1]
    stats = F.flow_consistency(fwd, bwd)[2]
    tight = F.flow_consistency(fwd, bwd, 0, 0)[2]
    print("16 x 16: stats %s at the defaults, %s at alpha = beta = 0" % (stats.tolist(), tight.tolist()))
    assert stats[0] > 0 and stats[2] > 0 and stats[1] == 0 and tight[1] > 0
