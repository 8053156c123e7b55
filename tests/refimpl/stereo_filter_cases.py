"""Inputs for the tests of vido_stereo_filter (tests/test_stereo_filter_cpu.py, tests/test_stereo_filter_gpu.py), each with the property of the statement's output that shows
the case is what its name says (so that a drifting generator cannot make a case vacuous).  A case is (name, q4 int32 [H,W], status uint8 [H,W], params, shows) with
shows(F, q4, status, params) -> bool, F = refimpl.stereo_filter_np."""
import numpy as np

from . import cc_patterns as P

RANDOM_SHAPES = ((1, 1), (1, 67), (67, 1), (31, 33), (33, 31), (97, 130))      # (H, W): below a tile, one pixel wide, odd, more than one tile both ways
TILE_SHAPES = ((64, 64), (32, 32))                                             # the GPU's extra shapes: four whole tiles, exactly one tile


def random_case(h, w, seed):
    """q4 in a narrow band around a few levels, so that edges exist at small thresholds and regions of every size appear; status mostly 0, the rest 1..3 and 200;
    a few status-0 pixels with q4 that is no disparity (0, negative, above 65535)"""
    rng = np.random.RandomState(seed)
    level = np.repeat(np.repeat(rng.randint(1, 40, ((h + 4) // 5, (w + 6) // 7)) * 24, 5, 0), 7, 1)[:h, :w]
    q4 = (level + rng.randint(-6, 7, (h, w))).astype(np.int32)
    q4[rng.rand(h, w) < 0.04] += 300
    status = np.where(rng.rand(h, w) < 0.8, 0, rng.choice(np.array([1, 2, 3, 200]), (h, w))).astype(np.uint8)
    for v in (0, -5, 65536, -2147483648, 2147483647):
        q4[rng.rand(h, w) < 0.01] = v
    return np.ascontiguousarray(q4), np.ascontiguousarray(status)


def random_cases(shapes=RANDOM_SHAPES, seed=11):
    out = []
    for k, (h, w) in enumerate(shapes):
        q4, status = random_case(h, w, seed + k)
        params = dict(max_diff_q4=8, min_region=6)
        def shows(F, q4=q4, status=status, params=params, big=h * w >= 900):
            _, st, _, stats = F.stereo_filter(q4, status, **params)
            # a large image holds removed and kept regions, copied statuses and bad q4 — a tiny one only has to run
            return not big or (stats[2] > 0 and stats[3] > 0 and (st == 200).any() and ((status == 0) & (st == 3)).any())
        out.append(("random %d x %d" % (h, w), q4, status, params, shows))
    return out


def pattern_masks(h, w):
    """every geometry of cc_patterns as a validity mask"""
    return [("blobs", P.blobs(h, w, 5)), ("full", P.full(h, w)), ("empty", P.empty(h, w)), ("checkerboard", P.checkerboard(h, w)), ("spirals", P.spirals(h, w)),
            ("serpentine", P.serpentine(h, w)), ("comb", P.comb(h, w)), ("corner_touch", P.corner_touch(h, w)), ("corner_touch anti", P.corner_touch(h, w, anti=True))]


def pattern_cases(h=97, w=130):
    """constant q4: the regions are the 4-connected components of the valid set.  Invalid pixels alternate between a copied status and a status-0 pixel without a disparity."""
    out = []
    yy, xx = np.mgrid[0:h, 0:w]
    for name, m in pattern_masks(h, w):
        v = m > 0
        q4 = np.where(v, 160, np.where((yy + xx) & 1, 0, 160)).astype(np.int32)
        status = np.where(v, 0, np.where((yy + xx) & 1, 0, 2)).astype(np.uint8)
        params = dict(max_diff_q4=0, min_region=40)
        out.append(("pattern " + name, q4, status, params, lambda F, q4=q4, status=status, v=v: np.array_equal(F.valid(q4, status), v)))
    return out


def column_ramp(h=33, w=67):
    """q4 = 16 (x + 1): one region at max_diff_q4 = 16 whose ends differ by 16 (w - 1); w regions of area h at 15"""
    q4 = np.broadcast_to(16 * (np.arange(w, dtype=np.int32) + 1), (h, w)).copy()
    return q4, np.zeros((h, w), np.uint8)


def boustrophedon(h=97, w=130):
    """q4 = 1 + 2 rank along the path that runs right on even rows and left on odd ones: vertical neighbours differ by 2 only at the row ends, so at max_diff_q4 = 2 the
    whole image is one region that exists only through the path; at 1 there is no edge at all"""
    yy, xx = np.mgrid[0:h, 0:w]
    rank = yy * w + np.where(yy & 1, w - 1 - xx, xx)
    return (1 + 2 * rank).astype(np.int32), np.zeros((h, w), np.uint8)


def ramp_cases():
    q4, st = column_ramp(); h, w = q4.shape
    bq, bs = boustrophedon(); n = bq.size
    def one(F, q4, status, t):
        A, area = F.region_areas(q4, status, t)
        return len(np.unique(A)) == 1 and int(area.max()) == q4.size
    return [
        ("column ramp, 16", q4, st, dict(max_diff_q4=16, min_region=h * w), lambda F: one(F, q4, st, 16)),
        ("column ramp, 15", q4, st, dict(max_diff_q4=15, min_region=h + 1), lambda F: (F.region_areas(q4, st, 15)[1] == h).all()),
        ("boustrophedon, 2", bq, bs, dict(max_diff_q4=2, min_region=n), lambda F: n == 12610 and one(F, bq, bs, 2)),
        ("boustrophedon, 2, one more", bq, bs, dict(max_diff_q4=2, min_region=n + 1), lambda F: one(F, bq, bs, 2)),
        ("boustrophedon, 1", bq, bs, dict(max_diff_q4=1, min_region=2), lambda F: not F.edges(bq, bs, 1)[0].any() and not F.edges(bq, bs, 1)[1].any()),
    ]


def sgm_case():
    """the SGM statement's own output on a warped pair: (q4, status) of stereo_cases.warped_pair(97, 66, 32, 3) at max_disp 32; the filter runs at (16, 20)"""
    from . import stereo_cases, stereo_sgm_np as G
    left, right = stereo_cases.warped_pair(97, 66, 32, 3)
    _, q4, status, _ = G.stereo_sgm(left, right, **{**G.DEFAULTS, "max_disp": 32})
    params = dict(max_diff_q4=16, min_region=20)
    def shows(F):
        stats = F.stereo_filter(q4, status, **params)[3]
        return stats[1] > 0 and stats[2] > 0 and stats[3] > 0
    return ("sgm output 97 x 66", q4, status, params, shows)


def all_cases():
    """every input of the GPU test: [(name, q4, status, params, shows(F) -> bool)]"""
    out = [(n, q, s, p, (lambda F, f=f: f(F))) for n, q, s, p, f in random_cases(RANDOM_SHAPES + TILE_SHAPES)]
    out += [(n, q, s, p, (lambda F, f=f: f(F))) for n, q, s, p, f in pattern_cases()]
    out += ramp_cases()
    out.append(sgm_case())
    return out
