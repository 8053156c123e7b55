"""The statement of vido_stereo_sgm (include/vido_c.h, csrc/stereosgm.hip): semi-global matching of a rectified pair, all in integers, numpy only.

  grey      1 channel: the bytes; 3 | 4: (1868 B + 9617 G + 4899 R + 8192) >> 14 (dis_flow_np.grey).
  census    window 9 wide x 7 high around the pixel, coordinates clamped to the image; the 62 neighbours row-major, the centre skipped; bit = neighbour < centre.
  cost      C(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)) for 0 <= d < D and x - d >= 0, 64 where x - d < 0.
  paths     eight directions r = (+-1, 0), (0, +-1), (+-1, +-1).  L_r(p, d) = C(p, d) where p - r lies outside the image (so a diagonal path restarts at the side columns);
            elsewhere, with m = min_k L_r(p - r, k): L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + p1, L_r(p - r, d + 1) + p1, m + p2) - m, a d +- 1 outside
            [0, D) being no candidate.  S = sum_r L_r.  L <= 64 + p2, S <= 8 (64 + p2).
  winner    d0 = argmin_d S(x, y, d), the lowest d on ties; s0 = S(d0).
  right     dR(x, y) = argmin_d S(x + d, y, d) over the d with x + d <= w - 1, the lowest d on ties.
  sub-pixel sm = S(d0 - 1), sp = S(d0 + 1), den = sm + sp - 2 s0; off = rdiv(8 (sm - sp), den) when 1 <= d0 <= D - 2 and den > 0, else 0 (rdiv: to the nearest, halves
            away from zero); q4 = 16 d0 + off, in 1/16 px.
  status    in this order: 2 (left-right) x - d0 < 0 or |dR(x - d0, y) - d0| > lr_tol; 1 (not unique) (100 - uniqueness) S2 <= 100 s0, S2 = min S(d) over |d - d0| > 1;
            3 (zero disparity) q4 <= 0; 0 otherwise.
  outputs   disp f32 = q4 / 16 where the status is 0, -1 elsewhere; q4 i32 of every pixel; status u8; stats i32 [4] = the count of each status.

stereo_sgm() is vectorised over d and across lines; stereo_sgm_loops() is the same rule pixel by pixel in Python integers, for small shapes (tests/test_stereo_sgm_cpu.py
holds the one against the other).  volumes() returns the intermediate planes for the bounds tests."""
import numpy as np

from .dis_flow_np import grey, rdiv

DEFAULTS = dict(max_disp=128, p1=10, p2=120, uniqueness=10, lr_tol=1)
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))          # (dx, dy)
BIG = 1 << 20

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def check_params(h, w, max_disp, p1, p2, uniqueness, lr_tol):
    if not (16 <= w <= 4095 and 16 <= h <= 4095):
        raise ValueError("16 <= w, h <= 4095 expected")
    if max_disp % 16 or not 16 <= max_disp <= 256 or w * h * max_disp > 1 << 28:
        raise ValueError("max_disp: a multiple of 16 in 16..256 with w * h * max_disp <= 2^28 expected")
    if not 0 <= p1 <= p2 <= 1000 or not 0 <= uniqueness <= 99 or not 0 <= lr_tol <= 255:
        raise ValueError("0 <= p1 <= p2 <= 1000, 0 <= uniqueness <= 99, 0 <= lr_tol <= 255 expected")


def popcount64(a):
    return _POP8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(-1).astype(np.int32)


def census(g):
    """g (h, w) integers -> (h, w) uint64; the first neighbour visited ends in the highest of the 62 bits used"""
    g = np.asarray(g, np.int64); h, w = g.shape
    p = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros((h, w), np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            out = (out << np.uint64(1)) | (p[3 + dy:3 + dy + h, 4 + dx:4 + dx + w] < g).astype(np.uint64)
    return out


def cost_volume(cl, cr, D):
    """(h, w, D) int32"""
    h, w = cl.shape
    C = np.full((h, w, D), 64, np.int32)
    for d in range(min(D, w)):
        C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :w - d])
    return C


def _step(C, Lp, ok, p1, p2):
    """One pixel further along n lines: C, Lp (n, D) = the costs here and L at the predecessors, ok (n,) = the predecessor is inside the image"""
    m = Lp.min(1, keepdims=True)
    best = np.minimum(Lp, m + p2)
    best[:, 1:] = np.minimum(best[:, 1:], Lp[:, :-1] + p1)
    best[:, :-1] = np.minimum(best[:, :-1], Lp[:, 1:] + p1)
    return np.where(ok[:, None], C + best - m, C)


def path(C, dx, dy, p1, p2):
    """L_r of one direction, (h, w, D) int32"""
    h, w, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], np.ones(h, bool), p1, p2)
        return L
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    xx = np.arange(w)
    ok = (xx - dx >= 0) & (xx - dx <= w - 1)
    src = np.clip(xx - dx, 0, w - 1)
    for i, y in enumerate(ys):
        L[y] = C[y] if i == 0 else _step(C[y], L[y - dy][src], ok, p1, p2)
    return L


def volumes(left, right, max_disp=128, p1=10, p2=120, rgb_order=0):
    """(C, [L_r of the eight directions], S), each (h, w, D) int32"""
    gl, gr = grey(left, rgb_order), grey(right, rgb_order)
    C = cost_volume(census(gl), census(gr), max_disp)
    Ls = [path(C, dx, dy, p1, p2) for dx, dy in DIRECTIONS]
    return C, Ls, sum(Ls)


def select(S, uniqueness, lr_tol):
    """S (h, w, D) -> (disp f32, q4 i32, status u8, stats i32 [4])"""
    h, w, D = S.shape
    S = S.astype(np.int64)
    d0 = S.argmin(2); s0 = S.min(2)
    dd = np.arange(D)
    SR = np.full((h, w, D), BIG, np.int64)
    for d in range(min(D, w)):
        SR[:, :w - d, d] = S[:, d:, d]
    dR = SR.argmin(2)
    take = lambda d: np.take_along_axis(S, np.clip(d, 0, D - 1)[..., None], 2)[..., 0]
    sm, sp = take(d0 - 1), take(d0 + 1)
    den = sm + sp - 2 * s0
    inner = (d0 >= 1) & (d0 <= D - 2) & (den > 0)
    off = np.where(inner, rdiv(8 * (sm - sp), np.where(inner, den, 1)), 0)
    q4 = 16 * d0 + off
    S2 = np.where(np.abs(dd[None, None, :] - d0[..., None]) > 1, S, BIG).min(2)
    xx = np.arange(w)[None, :] - d0
    yy = np.broadcast_to(np.arange(h)[:, None], (h, w))
    lr_bad = (xx < 0) | (np.abs(dR[yy, np.clip(xx, 0, w - 1)] - d0) > lr_tol)
    status = np.where(lr_bad, 2, np.where((100 - uniqueness) * S2 <= 100 * s0, 1, np.where(q4 <= 0, 3, 0))).astype(np.uint8)
    disp = np.where(status == 0, q4.astype(np.float32) / np.float32(16), np.float32(-1)).astype(np.float32)
    stats = np.bincount(status.ravel(), minlength=4).astype(np.int32)
    return disp, q4.astype(np.int32), status, stats


def stereo_sgm(left, right, max_disp=128, p1=10, p2=120, uniqueness=10, lr_tol=1, rgb_order=0):
    left, right = np.asarray(left), np.asarray(right)
    assert left.shape == right.shape
    check_params(left.shape[0], left.shape[1], max_disp, p1, p2, uniqueness, lr_tol)
    return select(volumes(left, right, max_disp, p1, p2, rgb_order)[2], uniqueness, lr_tol)


def stereo_sgm_loops(left, right, max_disp=128, p1=10, p2=120, uniqueness=10, lr_tol=1, rgb_order=0):
    """The same rule read literally: Python integers, one pixel and one disparity at a time.  Returns (disp, q4, status, stats, S)."""
    gl, gr = grey(left, rgb_order).tolist(), grey(right, rgb_order).tolist()
    h, w, D = len(gl), len(gl[0]), max_disp
    check_params(h, w, D, p1, p2, uniqueness, lr_tol)

    def cen(g, x, y):
        word = 0
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if dx or dy:
                    word = word << 1 | (g[min(max(y + dy, 0), h - 1)][min(max(x + dx, 0), w - 1)] < g[y][x])
        return word

    cl = [[cen(gl, x, y) for x in range(w)] for y in range(h)]
    cr = [[cen(gr, x, y) for x in range(w)] for y in range(h)]
    cost = lambda x, y, d: bin(cl[y][x] ^ cr[y][x - d]).count("1") if x - d >= 0 else 64
    S = [[[0] * D for _ in range(w)] for _ in range(h)]
    for dx, dy in DIRECTIONS:
        L = [[None] * w for _ in range(h)]
        for y in (range(h) if dy >= 0 else range(h - 1, -1, -1)):
            for x in (range(w) if dx >= 0 else range(w - 1, -1, -1)):
                px, py = x - dx, y - dy
                if px < 0 or px >= w or py < 0 or py >= h:
                    cur = [cost(x, y, d) for d in range(D)]
                else:
                    P = L[py][px]; m = min(P); cur = []
                    for d in range(D):
                        cand = [P[d], m + p2]
                        if d - 1 >= 0:
                            cand.append(P[d - 1] + p1)
                        if d + 1 < D:
                            cand.append(P[d + 1] + p1)
                        cur.append(cost(x, y, d) + min(cand) - m)
                L[y][x] = cur
                for d in range(D):
                    S[y][x][d] += cur[d]
    d0 = [[min(range(D), key=lambda d: (S[y][x][d], d)) for x in range(w)] for y in range(h)]
    dR = [[min((d for d in range(D) if x + d <= w - 1), key=lambda d: (S[y][x + d][d], d)) for x in range(w)] for y in range(h)]
    disp = np.empty((h, w), np.float32); q4 = np.empty((h, w), np.int32); status = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            d = d0[y][x]; s = S[y][x]; off = 0
            if 1 <= d <= D - 2:
                den = s[d - 1] + s[d + 1] - 2 * s[d]
                if den > 0:
                    a = 8 * (s[d - 1] - s[d + 1]); q, r = divmod(abs(a), den); q += r >= den - r
                    off = -q if a < 0 else q
            q = 16 * d + off
            S2 = min(s[k] for k in range(D) if abs(k - d) > 1)
            if x - d < 0 or abs(dR[y][x - d] - d) > lr_tol:
                st = 2
            elif (100 - uniqueness) * S2 <= 100 * s[d]:
                st = 1
            elif q <= 0:
                st = 3
            else:
                st = 0
            q4[y, x] = q; status[y, x] = st; disp[y, x] = q / 16.0 if st == 0 else -1.0
    return disp, q4, status, np.bincount(status.ravel(), minlength=4).astype(np.int32), np.array(S, np.int32)
