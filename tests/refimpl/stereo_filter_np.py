"""The statement of vido_stereo_filter (include/vido_c.h, csrc/stereofilter.hip): the speckle filter of a disparity image and the collision-depth plane, numpy only.

  valid     status == 0 and 1 <= q4 <= 65535.  A status-0 pixel with q4 outside that range gets status_out = 3; every other input status (values above 3 included) is
            copied through and is not valid.
  edge      two 4-neighbours (left / right, up / down), both valid, with |q4a - q4b| <= max_diff_q4.
  region    a connected component of the valid pixels under these edges; its area is its pixel count.  The relation is not transitive: a ramp is ONE region.
  speckle   a valid pixel whose region has area < min_region gets status_out = 4.
  outputs   status u8; disp f32 = q4 / 16 where status_out == 0, -1 elsewhere; depth f32 = bf / disp (one fp32 division) where status_out == 0, FLT_MAX elsewhere (None
            without bf); stats i32 [4] = valid pixels in, regions removed, pixels removed, valid pixels out.

How the regions are found (mask_components_np's scheme over this edge set): L[i] starts as i on valid pixels.  A round takes, for every pixel, the minimum m of L over
itself and the pixels it shares an edge with, hooks the pixel's current label under it (L[L[i]] = min(L[L[i]], m[i])), takes L = min(L, m), and replaces L by L[L] until
that changes nothing.  L[i] is always the index of a pixel of i's region and never grows; at the fixed point it is the region's smallest raster index, its anchor.
Nothing here is shared with the product (union-find in tiles, a seam merge, atomics)."""
import numpy as np

DEFAULTS = dict(max_diff_q4=16, min_region=10)      # chosen by tools/measure_stereo_filter.py's rule (profiles/r26/stereo_filter_cpu.txt)
FLT_MAX = np.float32(3.4028234663852886e38)
Q4_MAX = 65535


def check_params(h, w, max_diff_q4, min_region, bf=None):
    if not (1 <= w <= 4095 and 1 <= h <= 4095):
        raise ValueError("1 <= w, h <= 4095 expected")
    if not 0 <= max_diff_q4 <= 65535 or not 1 <= min_region <= 1 << 24:
        raise ValueError("0 <= max_diff_q4 <= 65535 and 1 <= min_region <= 2^24 expected")
    if bf is not None and not (np.isfinite(bf) and bf > 0):
        raise ValueError("bf: a finite value > 0 expected")


def valid(q4, status):
    q4 = np.asarray(q4); status = np.asarray(status)
    return (status == 0) & (q4 >= 1) & (q4 <= Q4_MAX)


def edges(q4, status, max_diff_q4):
    """-> (right [H, W-1] bool: pixel (y, x) shares an edge with (y, x + 1); down [H-1, W] bool: with (y + 1, x))"""
    v = valid(q4, status); q = np.asarray(q4).astype(np.int64)
    right = v[:, :-1] & v[:, 1:] & (np.abs(q[:, :-1] - q[:, 1:]) <= max_diff_q4)
    down = v[:-1, :] & v[1:, :] & (np.abs(q[:-1, :] - q[1:, :]) <= max_diff_q4)
    return right, down


def anchors(q4, status, max_diff_q4):
    """-> int64 [H,W]: the anchor (smallest raster index) of each valid pixel's region, -1 where the pixel is not valid."""
    q4 = np.asarray(q4); H, W = q4.shape
    v = valid(q4, status)
    right, down = edges(q4, status, max_diff_q4)
    big = H * W
    L = np.where(v, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
    pairs = [(slice(0, H), slice(0, W - 1), slice(0, H), slice(1, W), right), (slice(0, H - 1), slice(0, W), slice(1, H), slice(0, W), down)]
    pairs = [p for p in pairs if p[4].any()]
    fg = np.flatnonzero(v.ravel())
    while True:
        m = L.copy()
        for ya, xa, yb, xb, join in pairs:
            lo = np.where(join, np.minimum(L[ya, xa], L[yb, xb]), big)
            np.minimum(m[ya, xa], lo, out=m[ya, xa])
            np.minimum(m[yb, xb], lo, out=m[yb, xb])
        Lf, mf = L.ravel().copy(), m.ravel()
        np.minimum.at(Lf, L.ravel()[fg], mf[fg])                     # hook: the pixel's label goes under the smaller label it has seen
        Lf[fg] = np.minimum(Lf[fg], mf[fg])
        while True:                                                  # pointer jumping
            nxt = Lf.copy()
            nxt[fg] = Lf[Lf[fg]]
            if np.array_equal(nxt, Lf):
                break
            Lf = nxt
        Lf = Lf.reshape(H, W)
        if np.array_equal(Lf, L):
            break
        L = Lf
    return np.where(v, L, -1)


def region_areas(q4, status, max_diff_q4):
    """-> (anchors int64 [H,W], area int64 [H,W]: the area of each valid pixel's region, 0 where the pixel is not valid)"""
    A = anchors(q4, status, max_diff_q4)
    cnt = np.bincount(A[A >= 0], minlength=A.size + 1)
    return A, np.where(A >= 0, cnt[np.maximum(A, 0)], 0)


def stereo_filter(q4, status, max_diff_q4=DEFAULTS["max_diff_q4"], min_region=DEFAULTS["min_region"], bf=None):
    """q4 int32 [H,W], status uint8 [H,W] -> (disp f32 [H,W], status_out u8 [H,W], depth f32 [H,W] or None, stats i32 [4])"""
    q4 = np.asarray(q4); status = np.asarray(status)
    assert q4.ndim == 2 and q4.shape == status.shape
    check_params(q4.shape[0], q4.shape[1], max_diff_q4, min_region, bf)
    v = valid(q4, status)
    out = status.astype(np.uint8).copy()
    out[(status == 0) & ~v] = 3
    regions = pixels = 0
    if min_region > 1:
        A, area = region_areas(q4, status, max_diff_q4)
        small = v & (area < min_region)
        out[small] = 4
        pixels = int(small.sum()); regions = len(np.unique(A[small]))
    keep = out == 0
    disp = np.where(keep, q4.astype(np.float32) / np.float32(16), np.float32(-1)).astype(np.float32)
    depth = None
    if bf is not None:
        depth = np.full(q4.shape, FLT_MAX, np.float32)
        depth[keep] = np.float32(bf) / disp[keep]
    stats = np.array([int(v.sum()), regions, pixels, int(keep.sum())], np.int32)
    return disp, out, depth, stats
