"""The statement of vido_rectify_map and vido_rectify (include/vido_c.h), in numpy: a vectorised form and the rule read literally pixel by pixel.  Tests only.

Map (host, float64): for every destination pixel (u, v) of the rectified camera P = (fx', fy', cx', cy'), the raw pixel it shows, in 1/256 px.  Every operation is one
IEEE double operation in the order written below (numpy's element-wise operators fuse nothing); R (3 x 3, row-major) takes raw-camera to rectified coordinates, so the ray
of a rectified pixel goes back through R transposed.  No source: W <= 0, a value that is not finite, or |mx| or |my| >= 2^30 -> both entries INT32_MIN.

Remap (device, integers): bilinear in 1/256 px with the weights' product kept whole, (sum + 32768) >> 16; a pixel whose map entry lies outside
[0, (sw - 1) 256] x [0, (sh - 1) 256] is 0 in every channel and 0 in `inside`, and reads no source byte."""
import numpy as np

NO_SOURCE = np.int32(-2 ** 31)
LIMIT = float(2 ** 30)


def _params(K, dist, R, P):
    K, dist, R, P = (np.asarray(a, np.float64).ravel() for a in (K, dist, R, P))
    if K.size != 4 or dist.size != 5 or R.size != 9 or P.size != 4:
        raise ValueError("K[4], dist[5], R[9], P[4] expected")
    if not all(np.isfinite(a).all() for a in (K, dist, R, P)) or K[0] <= 0 or K[1] <= 0 or P[0] <= 0 or P[1] <= 0:
        raise ValueError("finite parameters with positive focal lengths expected")
    return K, dist, R, P


def _sizes(*sizes):
    for s in sizes:
        if not 16 <= int(s) <= 4095:
            raise ValueError("size %r outside 16 .. 4095" % (s,))


def inside_of(map_, src_w, src_h):
    """u8 [h, w]: 1 where the map entry lies in [0, (src_w - 1) 256] x [0, (src_h - 1) 256]"""
    mx, my = map_[..., 0].astype(np.int64), map_[..., 1].astype(np.int64)
    return ((mx >= 0) & (mx <= (src_w - 1) * 256) & (my >= 0) & (my <= (src_h - 1) * 256)).astype(np.uint8)


def rectify_map(K, dist, R, P, src_size, dst_size):
    """K, dist, R, P as in the header; src_size, dst_size = (w, h) -> (map int32 [dst_h, dst_w, 2] (x first), inside u8 [dst_h, dst_w])"""
    K, dist, R, P = _params(K, dist, R, P)
    (sw, sh), (dw, dh) = src_size, dst_size
    _sizes(sw, sh, dw, dh)
    fx, fy, cx, cy = K; k1, k2, p1, p2, k3 = dist; fxp, fyp, cxp, cyp = P
    u, v = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    with np.errstate(all="ignore"):
        x = (u - cxp) / fxp; y = (v - cyp) / fyp
        X = R[0] * x + R[3] * y + R[6]; Y = R[1] * x + R[4] * y + R[7]; W = R[2] * x + R[5] * y + R[8]
        xn = X / W; yn = Y / W; r2 = xn * xn + yn * yn
        rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = xn * rad + (2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)); yd = yn * rad + (p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn)
        us = fx * xd + cx; vs = fy * yd + cy
        mx = np.floor(us * 256 + 0.5); my = np.floor(vs * 256 + 0.5)
        ok = (W > 0) & np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) < LIMIT) & (np.abs(my) < LIMIT)
    m = np.full((dh, dw, 2), NO_SOURCE, np.int32)
    m[..., 0][ok] = mx[ok].astype(np.int32); m[..., 1][ok] = my[ok].astype(np.int32)
    return m, inside_of(m, sw, sh)


def rectify_map_loops(K, dist, R, P, src_size, dst_size):
    """the same, one pixel at a time on Python floats (IEEE doubles)"""
    import math
    K, dist, R, P = _params(K, dist, R, P)
    (sw, sh), (dw, dh) = src_size, dst_size
    _sizes(sw, sh, dw, dh)
    fx, fy, cx, cy = (float(a) for a in K); k1, k2, p1, p2, k3 = (float(a) for a in dist); fxp, fyp, cxp, cyp = (float(a) for a in P)
    R = [float(a) for a in R]
    m = np.empty((dh, dw, 2), np.int32); inside = np.zeros((dh, dw), np.uint8)
    div = lambda a, b: a / b if b != 0.0 else (math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b))
    for v in range(dh):
        for u in range(dw):
            x = (u - cxp) / fxp; y = (v - cyp) / fyp
            X = R[0] * x + R[3] * y + R[6]; Y = R[1] * x + R[4] * y + R[7]; W = R[2] * x + R[5] * y + R[8]
            xn = div(X, W); yn = div(Y, W); r2 = xn * xn + yn * yn
            rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
            xd = xn * rad + (2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)); yd = yn * rad + (p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn)
            us = fx * xd + cx; vs = fy * yd + cy
            a = us * 256 + 0.5; b = vs * 256 + 0.5
            if not (W > 0) or not math.isfinite(a) or not math.isfinite(b) or abs(math.floor(a)) >= LIMIT or abs(math.floor(b)) >= LIMIT:
                m[v, u] = NO_SOURCE
                continue
            m[v, u, 0] = math.floor(a); m[v, u, 1] = math.floor(b)
            inside[v, u] = 0 <= m[v, u, 0] <= (sw - 1) * 256 and 0 <= m[v, u, 1] <= (sh - 1) * 256
    return m, inside


def _image(src):
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3) or (src.ndim == 3 and src.shape[2] not in (1, 3, 4)):
        raise ValueError("a u8 image H x W or H x W x 1|3|4 expected")
    sh, sw = src.shape[:2]
    _sizes(sw, sh)
    return src, sw, sh


def rectify(src, map_):
    """src u8 [sh, sw] or [sh, sw, C], map int32 [h, w, 2] -> (out u8 [h, w] or [h, w, C], inside u8 [h, w])"""
    src, sw, sh = _image(src)
    map_ = np.asarray(map_)
    if map_.dtype != np.int32 or map_.ndim != 3 or map_.shape[2] != 2:
        raise ValueError("an int32 map [h, w, 2] expected")
    _sizes(map_.shape[1], map_.shape[0])
    inside = inside_of(map_, sw, sh)
    ok = inside.astype(bool)
    mx = np.where(ok, map_[..., 0], 0).astype(np.int64); my = np.where(ok, map_[..., 1], 0).astype(np.int64)
    x0 = mx >> 8; ax = mx & 255; x1 = np.minimum(x0 + 1, sw - 1)
    y0 = my >> 8; ay = my & 255; y1 = np.minimum(y0 + 1, sh - 1)
    s = src.reshape(sh, sw, -1).astype(np.int64)
    w00 = ((256 - ax) * (256 - ay))[..., None]; w01 = (ax * (256 - ay))[..., None]; w10 = ((256 - ax) * ay)[..., None]; w11 = (ax * ay)[..., None]
    acc = w00 * s[y0, x0] + w01 * s[y0, x1] + w10 * s[y1, x0] + w11 * s[y1, x1] + 32768
    assert acc.max() < 2 ** 31
    out = np.where(ok[..., None], acc >> 16, 0).astype(np.uint8)
    return out.reshape(map_.shape[:2] + src.shape[2:]), inside


def rectify_loops(src, map_):
    """the same, one pixel and one channel at a time"""
    src, sw, sh = _image(src)
    h, w = map_.shape[:2]
    s = src.reshape(sh, sw, -1); cn = s.shape[2]
    out = np.zeros((h, w, cn), np.uint8); inside = np.zeros((h, w), np.uint8)
    for v in range(h):
        for u in range(w):
            mx, my = int(map_[v, u, 0]), int(map_[v, u, 1])
            if not (0 <= mx <= (sw - 1) * 256 and 0 <= my <= (sh - 1) * 256):
                continue
            inside[v, u] = 1
            x0, ax, y0, ay = mx >> 8, mx & 255, my >> 8, my & 255
            x1, y1 = min(x0 + 1, sw - 1), min(y0 + 1, sh - 1)
            for c in range(cn):
                acc = ((256 - ax) * (256 - ay) * int(s[y0, x0, c]) + ax * (256 - ay) * int(s[y0, x1, c]) + (256 - ax) * ay * int(s[y1, x0, c]) + ax * ay * int(s[y1, x1, c]) + 32768)
                out[v, u, c] = acc >> 16
    return out.reshape((h, w) + src.shape[2:]), inside
