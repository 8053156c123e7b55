"""Inputs for the tests of vido_rectify_map / vido_rectify: rigs (calibrations of a raw camera and its rectified view), random images and hostile maps.  Tests only."""
import numpy as np

from . import stereo_rectify_np as G

KAIST_DIST = (-0.05004, 0.120012, -0.0006259, -0.00118, -0.063505)          # the reference's second configuration (Camera.k1, k2, p1, p2, k3)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def rodrigues(rx, ry, rz):
    """rotation vector -> 3 x 3 matrix"""
    r = np.array([rx, ry, rz], np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


R_LEFT = rodrigues(0.012, -0.017, 0.009)
R_RIGHT = rodrigues(-0.015, 0.011, -0.013)


def rig(w, h, which="left"):
    """The issue's rig scaled to a w x h raw frame (its 320 x 240 form has K = (250, 250, 159.5, 119.5), P = (235, 235, 159.5, 119.5)):
    dict(K, dist, R, P) for "left", "right", or "strong" (three times the rotation, twice the radial terms, anisotropic focal lengths)"""
    s = w / 320.0
    K = (250.0 * s, 250.0 * s, (w - 1) / 2.0, (h - 1) / 2.0); P = (235.0 * s, 235.0 * s, (w - 1) / 2.0, (h - 1) / 2.0)
    if which == "left":
        return dict(K=K, dist=KAIST_DIST, R=R_LEFT, P=P)
    if which == "right":
        return dict(K=K, dist=KAIST_DIST, R=R_RIGHT, P=P)
    if which == "strong":
        d = KAIST_DIST
        return dict(K=(K[0] * 1.03, K[1] * 0.98, K[2] + 1.75, K[3] - 2.25), dist=(2 * d[0], 2 * d[1], 3 * d[2], -2 * d[3], 2 * d[4]), R=rodrigues(0.036, -0.051, 0.027),
                    P=(P[0], P[1] * 1.01, P[2] - 0.5, P[3] + 0.25))
    raise ValueError(which)


RIGS = ("left", "right", "strong")


def behind_rig(w, h, deg=120.0):
    """R turns the view by `deg` degrees about y.  120: the whole rectified view looks behind the raw camera or so close to its horizon that the polynomial leaves
    every range (W <= 0, or beyond 2^30) -> the sentinel everywhere; 80: part of the view does, part of it has a source"""
    c = rig(w, h)
    return dict(c, R=rodrigues(0.0, np.deg2rad(deg), 0.0))


def image(w, h, cn, seed):
    """random u8 [h, w] (cn = 1) or [h, w, cn]"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w) if cn == 1 else (h, w, cn)).astype(np.uint8)


def smooth_map(sw, sh, dw, dh, seed):
    """An ordinary map: a random affine view of the source with a ripple, most of it inside, some of it beyond every edge"""
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    a = rng.uniform(-0.1, 0.1, 4)
    x = (sw - 1) * (u / (dw - 1) * 1.2 - 0.1) + a[0] * v + 1.5 * np.sin(v * 0.7 + a[1])
    y = (sh - 1) * (v / (dh - 1) * 1.2 - 0.1) + a[2] * u + 1.5 * np.cos(u * 0.9 + a[3])
    return np.stack([np.floor(x * 256 + 0.5), np.floor(y * 256 + 0.5)], -1).astype(np.int32)


def hostile_map(sw, sh, dw, dh, seed):
    """Every entry drawn from: the full int32 range (40 %), the source rectangle (30 %), and the values ON the rule's branches (30 %): INT32_MIN, INT32_MAX, -1, 0,
    (s - 1) 256 exactly (the last inside value: x1 = x0), (s - 1) 256 + 1 (the first outside value), (s - 1) 256 - 1, 255, 256.  x and y are drawn independently, so a
    special x meets an ordinary y and the reverse.  -> (map, census {name: count of pixels})"""
    rng = np.random.RandomState(seed)
    def axis(s):
        kind = rng.random_sample((dh, dw))
        full = rng.randint(INT32_MIN, INT32_MAX + 1, (dh, dw), dtype=np.int64)
        ordinary = rng.randint(0, (s - 1) * 256 + 1, (dh, dw), dtype=np.int64)
        special = np.array([INT32_MIN, INT32_MAX, -1, 0, (s - 1) * 256, (s - 1) * 256 + 1, (s - 1) * 256 - 1, 255, 256], np.int64)[rng.randint(0, 9, (dh, dw))]
        return np.where(kind < 0.4, full, np.where(kind < 0.7, ordinary, special))
    m = np.stack([axis(sw), axis(sh)], -1).astype(np.int32)
    mx, my = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    ins = G.inside_of(m, sw, sh).astype(bool)
    census = dict(inside=int(ins.sum()), outside=int((~ins).sum()), int_min=int(((mx == INT32_MIN) | (my == INT32_MIN)).sum()), int_max=int(((mx == INT32_MAX) | (my == INT32_MAX)).sum()),
                  minus_one=int(((mx == -1) | (my == -1)).sum()), last_inside=int((ins & ((mx == (sw - 1) * 256) | (my == (sh - 1) * 256))).sum()),
                  first_outside=int(((mx == (sw - 1) * 256 + 1) | (my == (sh - 1) * 256 + 1)).sum()),
                  outside_by_one_axis=int((~ins & (((mx >= 0) & (mx <= (sw - 1) * 256)) | ((my >= 0) & (my <= (sh - 1) * 256)))).sum()))
    return m, census


def planted_map(sw, sh, dw, dh):
    """A smooth map whose first pixels hold each special pair by name, whatever the seed: [(x, y)] at row 0, columns 0 .. """
    m = smooth_map(sw, sh, dw, dh, 3)
    ex, ey = (sw - 1) * 256, (sh - 1) * 256
    pairs = [(INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX), (-1, 0), (0, -1), (ex, ey), (ex + 1, ey), (ex, ey + 1), (0, 0), (ex, 0), (0, ey), (INT32_MIN, 0), (0, INT32_MAX),
                 (ex - 1, ey - 1), (255, 255)]
    for i, p in enumerate(pairs):
        m[i // dw, i % dw] = p
    return m, pairs
