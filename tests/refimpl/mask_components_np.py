"""Connected-component labelling of a class label image, stated in plain numpy: the reference of vido_mask_components (include/vido_c.h).

components(mask, connectivity=8, min_area=1, id_base=0, cap=127)
    -> (out int32 [H,W], classes int64 [cap], areas int32 [cap], stats int32 [4] = found, dropped for area, left out for cap, kept)

  mask     int32 [H,W]: > 0 a class (any positive value), <= 0 background
  1. a component is a maximal set of foreground pixels of EQUAL value joined by 4- or 8-neighbour steps; its anchor is its smallest raster index y * W + x, its area its
     pixel count
  2. components with area < min_area are dropped
  3. the survivors in ascending anchor order are k = 0, 1, ...; k < cap: out = id_base + 1 + k on its pixels, classes[k] = its value, areas[k] = its area; every other
     pixel of out is 0, every other entry of classes / areas is 0

How the labels are found.  L[i] starts as i on foreground.  A round takes, for every pixel, the minimum m of L over itself and its equal-valued neighbours, hooks the pixel's
current label under it (L[L[i]] = min(L[L[i]], m[i]): np.minimum.at), takes L = min(L, m), and then replaces L by L[L] until that changes nothing (pointer jumping).  L[i] is
always the index of a pixel of i's component and never grows, so the rounds end; at the fixed point every pixel equals its neighbours and points at itself's label, which is
then the component's minimum, the anchor.  Nothing here is shared with the product (csrc/maskcc.hip: union-find in tiles, a seam merge, atomics).
"""
import numpy as np

_STEPS4 = ((0, 1), (1, 0))
_STEPS8 = ((0, 1), (1, 0), (1, 1), (1, -1))


def anchors(mask, connectivity=8):
    """-> int64 [H,W]: the anchor (raster index) of each foreground pixel's component, -1 on background."""
    mask = np.asarray(mask)
    assert mask.dtype == np.int32 and mask.ndim == 2 and connectivity in (4, 8)
    H, W = mask.shape
    fg = mask > 0
    big = H * W
    L = np.where(fg, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
    pairs = []                                                       # (slice of a, slice of b, a and b are joined) per half of the neighbourhood
    for dy, dx in (_STEPS8 if connectivity == 8 else _STEPS4):
        ya, yb = slice(0, H - dy), slice(dy, H)
        xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        join = fg[ya, xa] & (mask[ya, xa] == mask[yb, xb])
        if join.any():
            pairs.append((ya, xa, yb, xb, join))
    flat_fg = np.flatnonzero(fg.ravel())
    while True:
        m = L.copy()
        for ya, xa, yb, xb, join in pairs:
            a, b = L[ya, xa], L[yb, xb]
            lo = np.minimum(a, b)
            np.minimum(m[ya, xa], np.where(join, lo, big), out=m[ya, xa])
            np.minimum(m[yb, xb], np.where(join, lo, big), out=m[yb, xb])
        Lf, mf = L.ravel().copy(), m.ravel()
        np.minimum.at(Lf, L.ravel()[flat_fg], mf[flat_fg])           # hook: the pixel's label goes under the smaller label it has seen
        Lf[flat_fg] = np.minimum(Lf[flat_fg], mf[flat_fg])
        while True:                                                  # pointer jumping
            nxt = Lf.copy()
            nxt[flat_fg] = Lf[Lf[flat_fg]]
            if np.array_equal(nxt, Lf):
                break
            Lf = nxt
        Lf = Lf.reshape(H, W)
        if np.array_equal(Lf, L):
            break
        L = Lf
    return np.where(fg, L, -1)


def components(mask, connectivity=8, min_area=1, id_base=0, cap=127):
    assert id_base >= 0 and cap >= 1 and id_base + cap <= 254
    mask = np.asarray(mask)
    A = anchors(mask, connectivity)
    H, W = mask.shape
    roots, area = np.unique(A[A >= 0], return_counts=True)           # ascending anchors
    found = len(roots)
    keep = area >= min_area
    roots, area = roots[keep], area[keep]
    surv = len(roots)
    kept = min(surv, cap)
    classes = np.zeros(cap, np.int64); areas = np.zeros(cap, np.int32)
    classes[:kept] = mask.ravel()[roots[:kept]]
    areas[:kept] = area[:kept]
    ids = np.zeros(H * W + 1, np.int32)                              # by anchor; the last entry serves background (-1)
    ids[roots[:kept]] = id_base + 1 + np.arange(kept, dtype=np.int32)
    out = ids[A]
    return out, classes, areas, np.array([found, found - surv, surv - kept, kept], np.int32)
