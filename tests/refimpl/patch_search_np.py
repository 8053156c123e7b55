"""The statement of vido_orb_patch_search in numpy and Python integers (no GPU, no float): the offset inside a square window at which the 8 x 8 patch of a pyramid level
correlates best with a reference patch, the runner-up outside the winner's own peak, and a verdict.  csrc/patchsearch.hip must equal every output bit for bit.

Point k = (x, y, level) in level coordinates with the 64-byte reference patch a.  Patches, the three sums (cov, var_ref, var_cur) and the rule "wholly inside the level" are
those of patch_points_np (take / sums).  In the order the rules apply:
    candidates   the offsets (dx, dy), |dx| <= radius, |dy| <= radius, whose patch at (x + dx, y + dy) lies wholly inside the level
    status -1    level out of range or no candidate: every output of the point is 0
    status  2    var_ref < min_var (no texture in the reference): nothing is searched; sums = (0, var_ref, 0), the rest 0
    eligible     a candidate with var_cur >= min_var and cov > 0
    order        p before q iff cov_p^2 var_q > cov_q^2 var_p (ZNCC^2, var_ref being common); on equality the smaller dx^2 + dy^2, then the smaller dy, then the smaller dx
    best         the first eligible candidate in that order; none: status 1, dxy = 0, sums = (0, var_ref, 0), second = 0
    dxy, sums    the best's offset and its (cov, var_ref, var_cur)
    second       (cov, var_cur) of the first eligible candidate in that order with max(|dx - dx1|, |dy - dy1|) > excl; (0, 0) if there is none.  It is reported whenever
                 there is a best, whatever the status
    status  1    the best fails cov^2 1024^2 >= min_zncc_q10^2 var_ref var_cur                        (patch_points_np.verdict's gate: equality accepts)
    status  3    else, with peak_ratio_q10 > 0 and a second: cov2^2 var1 1024^2 > peak_ratio_q10^2 cov1^2 var2        (ZNCC2 > r ZNCC1: ambiguous)
    status  0    otherwise
stats[0..3] count the statuses 0..3, stats[4] counts status -1.  All comparisons are on exact integers (each side below 2^98)."""
import numpy as np

from .patch_points_np import sums as _sums, take as _take

MAX_RADIUS = 16


def check_params(radius, excl, min_var, min_zncc_q10, peak_ratio_q10):
    if not 0 <= radius <= MAX_RADIUS or not 1 <= excl <= 16 or min_var < 0 or not 0 <= min_zncc_q10 <= 1024 or not 0 <= peak_ratio_q10 <= 1024:
        raise ValueError("radius in 0..16, excl in 1..16, min_var >= 0, min_zncc_q10 and peak_ratio_q10 in 0..1024 expected")


def before(p, q):
    """p, q = (cov, var_cur, dx, dy) of two eligible candidates: True iff p comes first in the order"""
    l, r = p[0] * p[0] * q[1], q[0] * q[0] * p[1]
    if l != r:
        return l > r
    return (p[2] * p[2] + p[3] * p[3], p[3], p[2]) < (q[2] * q[2] + q[3] * q[3], q[3], q[2])


def _first(cands):
    best = None
    for c in cands:
        if best is None or before(c, best):
            best = c
    return best


def search_one(levels, x, y, level, a, radius, excl, min_var, min_zncc_q10, peak_ratio_q10):
    """(status, (dx, dy), (cov, var_ref, var_cur), (cov2, var2)) of one point, Python integers"""
    check_params(radius, excl, min_var, min_zncc_q10, peak_ratio_q10)
    x, y, level = int(x), int(y), int(level)
    zero = (-1, (0, 0), (0, 0, 0), (0, 0))
    if not 0 <= level < len(levels):
        return zero
    offs = [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    h, w = levels[level].shape
    vx = [4 <= x + d and x + d + 3 < w for d in range(-radius, radius + 1)]; vy = [4 <= y + d and y + d + 3 < h for d in range(-radius, radius + 1)]      # take's rule
    valid = np.outer(vy, vx).reshape(-1)
    if not valid.any():
        return zero
    # every candidate's patch at once: the 8 x 8 windows of the part of the level that the valid candidates cover, dy-major like offs
    x0 = x - radius + vx.index(True); y0 = y - radius + vy.index(True)
    region = levels[level][y0 - 4:y0 + sum(vy) + 3, x0 - 4:x0 + sum(vx) + 3]
    patch = np.zeros((len(offs), 64), np.uint8)
    patch[valid] = np.lib.stride_tricks.sliding_window_view(region, (8, 8)).reshape(-1, 64)
    var_ref = _sums(a, a)[1]
    if var_ref < min_var:
        return 2, (0, 0), (0, var_ref, 0), (0, 0)
    # the three sums of every candidate at once in int64 (exact: below 2^29); patch_points_np.sums is the definition, and the two candidates that decide are held to it
    A = np.asarray(a, np.uint8).reshape(64).astype(np.int64); Bm = patch.astype(np.int64)
    s1 = int(A.sum()); s2 = Bm.sum(1); cov_all = 64 * (Bm @ A) - s1 * s2; var_all = 64 * (Bm * Bm).sum(1) - s2 * s2
    elig = [(int(cov_all[i]), int(var_all[i]), offs[i][0], offs[i][1]) for i in np.flatnonzero(valid & (var_all >= min_var) & (cov_all > 0))]
    b1 = _first(elig)
    if b1 is None:
        return 1, (0, 0), (0, var_ref, 0), (0, 0)
    b2 = _first([c for c in elig if max(abs(c[2] - b1[2]), abs(c[3] - b1[3])) > excl])
    second = (b2[0], b2[1]) if b2 is not None else (0, 0)
    for c in (b1, b2):                                                           # the two that decide, by the definition itself
        if c is not None:
            pc, ok = _take(levels, [(x + c[2], y + c[3], level)])
            assert ok[0] and _sums(a, pc[0]) == (c[0], var_ref, c[1])
    cov1, var1 = b1[0], b1[1]
    if not cov1 * cov1 * 1024 * 1024 >= min_zncc_q10 * min_zncc_q10 * var_ref * var1:
        st = 1
    elif peak_ratio_q10 > 0 and b2 is not None and b2[0] * b2[0] * var1 * 1024 * 1024 > peak_ratio_q10 * peak_ratio_q10 * cov1 * cov1 * b2[1]:
        st = 3
    else:
        st = 0
    return st, (b1[2], b1[3]), (cov1, var_ref, var1), second


def patch_search(levels, xyl, ref_patch, radius, excl=2, min_var=147456, min_zncc_q10=920, peak_ratio_q10=0):
    """(dxy (n,2) i32, sums (n,3) i32, second (n,2) i32, status (n,) i32, stats (5,) i32): the five outputs of vido_orb_patch_search"""
    check_params(radius, excl, min_var, min_zncc_q10, peak_ratio_q10)
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3); n = len(xyl)
    ref = np.asarray(ref_patch, np.uint8).reshape(n, 64)
    dxy = np.zeros((n, 2), np.int32); sm = np.zeros((n, 3), np.int32); sec = np.zeros((n, 2), np.int32); st = np.zeros(n, np.int32); stats = np.zeros(5, np.int32)
    for k in range(n):
        st[k], dxy[k], sm[k], sec[k] = search_one(levels, xyl[k, 0], xyl[k, 1], xyl[k, 2], ref[k], radius, excl, min_var, min_zncc_q10, peak_ratio_q10)
        stats[st[k] if st[k] >= 0 else 4] += 1
    return dxy, sm, sec, st, stats
