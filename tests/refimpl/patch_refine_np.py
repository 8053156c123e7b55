"""The statement of vido_orb_patch_refine in numpy and Python integers (no GPU, no float): translation-only inverse-compositional alignment, with a bias term, of a
carried 8 x 8 reference patch to a pyramid level, to 1/256 px.  csrc/patchrefine.hip must equal every output bit for bit.

Point k = (x, y, level) in level coordinates with the 64-byte reference patch T[r][c], r, c in 0..7; T[r][c] belongs to level pixel (x - 4 + c, y - 4 + r) (the take rule
of patch_points_np).  Only the 36 interior pixels r, c in 1..6 are compared (n = 36 below); the border ring serves the template's gradients.  Parameters: iters in 1..8,
max_shift_q8 in 0..512 (1/256 px), min_eig >= 0.  In the order the rules apply:
    status -1    level out of range, or not (x - 3 - C >= 0 and x + 3 + C <= w - 1 and the same in y) with C = (max_shift_q8 + 255) >> 8: every output of the point is 0.
                 Otherwise the footprint is inside the level for every admissible offset; no iterate is clamped or checked again
    gradients    gx = T[r][c+1] - T[r][c-1], gy = T[r+1][c] - T[r-1][c]                           (twice the central difference)
    Hessian      Hxx = n sum gx^2 - (sum gx)^2, Hyy = n sum gy^2 - (sum gy)^2, Hxy = n sum gx gy - sum gx sum gy, det = Hxx Hyy - Hxy^2, tr = Hxx + Hyy
    status  2    det <= 0 or tr < 2 min_eig or det - min_eig tr + min_eig^2 < 0 (the smaller eigenvalue of H is below min_eig, without a root: no texture, or an edge
                 only): q8 = 0, cost = (0, 0), iters = 0
    evaluation   at offset p = (px, py) in 1/256 px: X = (x - 4 + c) 256 + px, ix = X >> 8, fx = X & 255 (Y, iy, fy likewise; >> is arithmetic),
                 I = (256 - fx)(256 - fy) L[iy][ix] + fx (256 - fy) L[iy][ix+1] + (256 - fx) fy L[iy+1][ix] + fx fy L[iy+1][ix+1]
                 e = (I - 65536 T[r][c] + 128) >> 8, cost = n sum e^2 - (sum e)^2, bx = n sum gx e - sum gx sum e, by = n sum gy e - sum gy sum e
    step         numx = Hyy bx - Hxy by, numy = Hxx by - Hxy bx, dx = rdiv(-2 numx, det), dy = rdiv(-2 numy, det), each clamped to +-256;
                 rdiv(a, d): q = |a| div d, r = |a| mod d, q += (r >= d - r), with the sign of a
    loop         p = (0, 0), cost0 = cost(p); at most iters times: step; (dx, dy) = (0, 0) stops; p += (dx, dy); |px| > max_shift_q8 or |py| > max_shift_q8 is
                 status 3 (q8 = 0, cost = (cost0, cost0)); else the cost is evaluated at the new p (also after the last step)
    status  0    q8 = the iterate of the smallest cost, the earliest on ties; cost = (cost0, cost_best)
    iters        the number of steps taken (p += ...), the one that left the window included
stats[0..3] count the statuses 0, 2, 3, -1.

Bounds (all arithmetic fits int64): |e| <= 65 280, |g| <= 255; sum e, sum g e, sum g^2 fit int32, sum e^2 < 2^37.2; |b| = n^2 |cov(g, e)| <= 36 36 255 65 280 < 2^34.4;
H = n^2 var(g) <= 36^2 255^2 < 2^26.4; det < 2^52.7 < 2^53; |num| <= 2 * 2^26.4 * 2^34.4, |2 num| < 2^62.7; cost <= 36^2 65 280^2 < 2^42.4;
min_eig < 2^31: min_eig tr < 2^58.4, min_eig^2 < 2^62."""
import numpy as np

N = 36
MAX_ITERS = 8
MAX_SHIFT_Q8 = 512


def check_params(iters, max_shift_q8, min_eig):
    if not 1 <= iters <= MAX_ITERS or not 0 <= max_shift_q8 <= MAX_SHIFT_Q8 or min_eig < 0:
        raise ValueError("iters in 1..8, max_shift_q8 in 0..512, min_eig >= 0 expected")


def rdiv(a, d):
    """a / d rounded to the nearest, halves away from zero; d > 0"""
    q, r = divmod(abs(a), d)
    q += r >= d - r
    return -q if a < 0 else q


def hessian(T):
    """(gx, gy (36,) int64, sgx, sgy, Hxx, Hyy, Hxy, det, tr) of a 64-byte reference patch, Python integers"""
    T = np.asarray(T, np.uint8).reshape(8, 8).astype(np.int64)
    gx = (T[1:7, 2:8] - T[1:7, 0:6]).reshape(36); gy = (T[2:8, 1:7] - T[0:6, 1:7]).reshape(36)
    sgx, sgy = int(gx.sum()), int(gy.sum())
    hxx = N * int((gx * gx).sum()) - sgx * sgx; hyy = N * int((gy * gy).sum()) - sgy * sgy; hxy = N * int((gx * gy).sum()) - sgx * sgy
    return gx, gy, sgx, sgy, hxx, hyy, hxy, hxx * hyy - hxy * hxy, hxx + hyy


def gated(det, tr, min_eig):
    return det <= 0 or tr < 2 * min_eig or det - min_eig * tr + min_eig * min_eig < 0


def evaluate(L, x, y, T36, gx, gy, sgx, sgy, px, py):
    """(cost, bx, by, max |e|) at offset (px, py), Python integers; L = the level as int64"""
    X = (x - 4 + np.arange(1, 7, dtype=np.int64)) * 256 + px; Y = (y - 4 + np.arange(1, 7, dtype=np.int64)) * 256 + py
    ix, fx, iy, fy = X >> 8, X & 255, (Y >> 8)[:, None], (Y & 255)[:, None]
    I = (256 - fx) * (256 - fy) * L[iy, ix] + fx * (256 - fy) * L[iy, ix + 1] + (256 - fx) * fy * L[iy + 1, ix] + fx * fy * L[iy + 1, ix + 1]
    e = ((I.reshape(36) - 65536 * T36 + 128) >> 8)
    se, see, sxe, sye = int(e.sum()), int((e * e).sum()), int((gx * e).sum()), int((gy * e).sum())
    return N * see - se * se, N * sxe - sgx * se, N * sye - sgy * se, int(np.abs(e).max())


def refine_one(levels, x, y, level, T, iters, max_shift_q8, min_eig, trace=None):
    """(status, (qx, qy), (cost0, cost_best), steps) of one point, Python integers.  trace: a dict that collects the largest magnitudes met (max_e, max_b, max_h, max_det,
    max_2num, max_cost) and the iterates (path)"""
    check_params(iters, max_shift_q8, min_eig)
    x, y, level = int(x), int(y), int(level)
    if not 0 <= level < len(levels):
        return -1, (0, 0), (0, 0), 0
    h, w = levels[level].shape; C = (max_shift_q8 + 255) >> 8
    if not (x - 3 - C >= 0 and x + 3 + C <= w - 1 and y - 3 - C >= 0 and y + 3 + C <= h - 1):
        return -1, (0, 0), (0, 0), 0
    gx, gy, sgx, sgy, hxx, hyy, hxy, det, tr = hessian(T)
    note = (lambda k, v: trace.__setitem__(k, max(trace.get(k, 0), abs(v)))) if trace is not None else (lambda k, v: None)
    note("max_h", max(hxx, hyy, abs(hxy))); note("max_det", det)
    if gated(det, tr, min_eig):
        return 2, (0, 0), (0, 0), 0
    L = levels[level].astype(np.int64); T36 = np.asarray(T, np.uint8).reshape(8, 8)[1:7, 1:7].reshape(36).astype(np.int64)
    px = py = 0; steps = 0
    cost, bx, by, me = evaluate(L, x, y, T36, gx, gy, sgx, sgy, px, py)
    cost0 = cost; best = (cost, px, py)
    path = [(px, py, cost)]
    for _ in range(iters):
        numx, numy = hyy * bx - hxy * by, hxx * by - hxy * bx
        note("max_e", me); note("max_b", max(abs(bx), abs(by))); note("max_2num", 2 * max(abs(numx), abs(numy))); note("max_cost", cost)
        dx = min(max(rdiv(-2 * numx, det), -256), 256); dy = min(max(rdiv(-2 * numy, det), -256), 256)
        if dx == 0 and dy == 0:
            break
        px += dx; py += dy; steps += 1
        if abs(px) > max_shift_q8 or abs(py) > max_shift_q8:
            return 3, (0, 0), (cost0, cost0), steps
        cost, bx, by, me = evaluate(L, x, y, T36, gx, gy, sgx, sgy, px, py)
        path.append((px, py, cost))
        if cost < best[0]:
            best = (cost, px, py)
    if trace is not None:
        trace["path"] = path
    return 0, (best[1], best[2]), (cost0, best[0]), steps


def patch_refine(levels, xyl, ref, iters, max_shift_q8, min_eig):
    """(q8 (n,2) i32, cost (n,2) i64, iters (n,) i32, status (n,) i32, stats (4,) i32): the five outputs of vido_orb_patch_refine"""
    check_params(iters, max_shift_q8, min_eig)
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3); n = len(xyl)
    ref = np.asarray(ref, np.uint8).reshape(n, 64)
    q8 = np.zeros((n, 2), np.int32); cost = np.zeros((n, 2), np.int64); it = np.zeros(n, np.int32); st = np.zeros(n, np.int32); stats = np.zeros(4, np.int32)
    for k in range(n):
        st[k], q8[k], cost[k], it[k] = refine_one(levels, xyl[k, 0], xyl[k, 1], xyl[k, 2], ref[k], iters, max_shift_q8, min_eig)
        stats[{0: 0, 2: 1, 3: 2, -1: 3}[int(st[k])]] += 1
    return q8, cost, it, st, stats


def resample(L, x, y, px, py):
    """The 8 x 8 patch of level L around (x, y) at offset (px, py) in 1/256 px by the statement's own bilinear form, rounded to bytes: (I + 32768) >> 16"""
    L = np.asarray(L).astype(np.int64)
    X = (x - 4 + np.arange(8, dtype=np.int64)) * 256 + px; Y = (y - 4 + np.arange(8, dtype=np.int64)) * 256 + py
    ix, fx, iy, fy = X >> 8, X & 255, (Y >> 8)[:, None], (Y & 255)[:, None]
    I = (256 - fx) * (256 - fy) * L[iy, ix] + fx * (256 - fy) * L[iy, ix + 1] + (256 - fx) * fy * L[iy + 1, ix] + fx * fy * L[iy + 1, ix + 1]
    return ((I + 32768) >> 16).astype(np.uint8).reshape(64)


TILE = 16                     # constructed(): every image is a TILE x TILE level with the point at (8, 8)
KNOWN_OFFSET = (64, -96)


def smooth_tile(seed=5):
    """A TILE x TILE byte image of full contrast whose structure is a few pixels wide: random values on a 3-px grid, bilinearly upsampled"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 256, (TILE // 3 + 2, TILE // 3 + 2)).astype(np.float64)
    yy, xx = np.mgrid[0:TILE, 0:TILE] / 3.0
    y0, x0 = yy.astype(int), xx.astype(int); ay, ax = yy - y0, xx - x0
    v = (1 - ay) * (1 - ax) * g[y0, x0] + (1 - ay) * ax * g[y0, x0 + 1] + ay * (1 - ax) * g[y0 + 1, x0] + ay * ax * g[y0 + 1, x0 + 1]
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def constructed():
    """name -> dict(ref (64,) u8, img (TILE, TILE) u8, the point is (8, 8, 0); iters, max_shift_q8, min_eig; status, and q8 / steps where the definition gives them):
    the cases whose result follows from the statement alone"""
    rng = np.random.RandomState(7)
    rnd = rng.randint(0, 256, (TILE, TILE)).astype(np.uint8)
    yy, xx = np.mgrid[0:TILE, 0:TILE]
    cut = lambda img, dx=0, dy=0: img[4 + dy:12 + dy, 4 + dx:12 + dx].reshape(64).copy()               # the patch of (8 + dx, 8 + dy)
    checker = ((((yy >> 1) + (xx >> 1)) & 1) * 255).astype(np.uint8)                                   # 2-px squares: every gx, gy is +-255 and sums to 0: H = 36^2 255^2
    vedge = np.where(xx < 8, 0, 255).astype(np.uint8)                                                  # gy = 0: Hyy = 0, det = 0
    ramp = (10 * xx + 5 * yy + 20).astype(np.uint8)                                                    # gx, gy constant: H = 0 (the bias term takes a ramp's slope away)
    bowl = ((xx * xx + yy * yy) // 2).astype(np.uint8)                                                 # gradients linear in x, y: a Gauss-Newton step lands on the offset
    smooth = smooth_tile()
    base = dict(iters=6, max_shift_q8=384, min_eig=0)
    return {
        "flat": dict(base, ref=np.full(64, 17, np.uint8), img=rnd, status=2),
        "vertical_edge": dict(base, ref=cut(vedge), img=vedge, status=2),
        "ramp": dict(base, ref=cut(ramp), img=ramp, status=2),
        "checker": dict(base, ref=cut(checker), img=checker, status=0, q8=(0, 0), steps=0),
        "checker_inverse": dict(base, ref=cut(checker), img=(255 - checker).astype(np.uint8), status=None),        # |e| = 65 280 everywhere: the largest operands
        "checker_shifted": dict(base, ref=cut(checker), img=np.roll(checker, 1, axis=1), status=None),                    # e = +-65 280 on half of the pixels, in step with gx: a large b
        "leaves_window": dict(base, ref=cut(bowl, 3, 0), img=bowl, status=3, steps=2),                             # 3 px away: two clamped steps of 256 pass 384
        "known_offset": dict(base, ref=resample(smooth, 8, 8, *KNOWN_OFFSET), img=smooth, status=0, q8=KNOWN_OFFSET),
    }
