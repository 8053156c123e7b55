"""The statement of vido_dis_flow in numpy and Python integers (no GPU, no float): dense optical flow of the Dense Inverse Search kind — translation-only
inverse-compositional alignment, with a bias term, of every 8 x 8 patch of image 0 to image 1 on a coarse-to-fine pyramid, densified by photometric-weighted averaging —
to 1/256 px.  csrc/disflow.hip must equal every output bit for bit.  Vectorised over patches and pixels: a 640 x 480 pair takes seconds.

Inputs: two u8 images of one size, 16 <= w, h <= 4095, H x W or H x W x 3|4 (rgb_order as in vido_orb_extract_color: 0 = B first, else R first).  Parameters: coarsest L in
0..6 with min(w, h) >> L >= 8, iters in 1..16, max_shift_q8 in 0..2048 (1/256 px), min_eig >= 0 (< 2^31).  In the order the rules apply:
    grey         1 channel: the bytes; 3 | 4 channels: (1868 B + 9617 G + 4899 R + 8192) >> 14 (the bits of k_ingest_color)
    pyramid      G[l+1][y][x] = (G[l][2y][2x] + G[l][2y][2x+1] + G[l][2y+1][2x] + G[l][2y+1][2x+1] + 2) >> 2, w[l+1] = w[l] >> 1, h likewise, of both images
    flow         U[l][y][x] = (ux, uy) int32 in 1/256 px of level l; levels L .. 0; the initial field is 0 at level L and 2 U[l+1][min(y >> 1, h[l+1] - 1)][min(x >> 1,
                 w[l+1] - 1)] below
    patches      8 x 8 with origin (x0, y0); along an axis of length n the origins are 0, 4, 8, ... while o + 8 <= n, plus n - 8 when that is not among them (a pixel is
                 in 1..9 patches); u0 = the initial field at (x0 + 4, y0 + 4)
    template     N = 64 pixels; T = the patch of image 0; gx = G0[y][min(x+1, w-1)] - G0[y][max(x-1, 0)], gy likewise (twice the central difference, of the IMAGE);
                 Hxx = N sum gx^2 - (sum gx)^2, Hyy, Hxy likewise, det = Hxx Hyy - Hxy^2, tr = Hxx + Hyy; flat when patch_refine_np.gated(det, tr, min_eig): keeps u0
    sample       S(X, Y) of image 1 at Q8 level coordinates: X clamped to [0, (w-1) 256], ix = X >> 8, fx = X & 255, right neighbour min(ix+1, w-1), y likewise;
                 S = (256-fx)(256-fy) a + fx (256-fy) b + (256-fx) fy c + fx fy d (weights sum to 65536)
    evaluation   at u: e = (S((x0+c) 256 + ux, (y0+r) 256 + uy) - 65536 T[r][c] + 2048) >> 12 (1/16 grey, |e| <= 4080); cost = N sum e^2 - (sum e)^2,
                 bx = N sum gx e - sum gx sum e, by likewise
    step         d = (rdiv(-32 (Hyy bx - Hxy by), det), rdiv(-32 (Hxx by - Hxy bx), det)) with patch_refine_np.rdiv, each component clamped to +-256.  (32, where
                 patch_refine_np has 2: e is in 1/16 grey here and in 1/256 grey there, and the step is in 1/256 px in both.  32 |num| can pass 2^63, so it is
                 taken in two divisions that stay in int64 and give the same integer: |2 num| = q1 det + r1, then 16 min(q1, 17) + rdiv(16 r1, det), 16 r1 < 2^60)
    loop         u = u0, cost(u0); at most iters times: step; d = (0, 0) stops; u += d; max(|ux - u0x|, |uy - u0y|) > max_shift_q8: the patch is rejected and keeps u0;
                 else the cost is evaluated at the new u (also after the last step).  The iterate of the smallest cost wins, the earliest on ties
    densify      level l, pixel (x, y), over every patch p that contains it: d = |S(x 256 + u_p.x, y 256 + u_p.y) - 65536 G0[y][x]| >> 16, wgt = 65536 // max(1, d),
                 U = (rdiv(sum wgt u_p.x, sum wgt), rdiv(sum wgt u_p.y, sum wgt))
Outputs: q8 int32 [h][w][2] = U[0]; flow f32 = q8 / 256 (exact: |q8| < 2^19); stats int32 [4], summed over the levels: patches that kept an iterate, flat patches,
rejected patches, steps taken (u += d; the one that left the window included).

Bounds (all arithmetic fits int64): |g| <= 255, |e| <= 4080; sums of e, g e, g^2, e^2 over 64 pixels fit int32 except sum e^2 <= 64 4080^2 < 2^30.1 (fits too);
H <= 64^2 255^2 < 2^28; |b| <= 64^2 255 4080 < 2^32; det < 2^56; |num| <= 2 2^28 2^32, |2 num| < 2^62; cost <= 64^2 4080^2 < 2^36; min_eig tr < 2^60,
min_eig^2 < 2^62; |u| <= 2048 (2^(L+1) - 1) < 2^19; densify: sum wgt <= 9 65536, |sum wgt u| < 2^39."""
import numpy as np

N = 64
MAX_ITERS = 16
MAX_SHIFT_Q8 = 2048
MAX_COARSEST = 6
DEFAULTS = dict(coarsest=4, iters=6, max_shift_q8=1024, min_eig=0)
BOUNDS = dict(max_e=4080, max_h=64 * 64 * 255 * 255, max_b=64 * 64 * 255 * 4080, max_2num=1 << 62, max_cost=64 * 64 * 4080 * 4080)


def check_params(h, w, coarsest, iters, max_shift_q8, min_eig):
    if not (16 <= w <= 4095 and 16 <= h <= 4095):
        raise ValueError("16 <= w, h <= 4095 expected")
    if not 0 <= coarsest <= MAX_COARSEST or (min(w, h) >> coarsest) < 8:
        raise ValueError("coarsest in 0..6 with min(w, h) >> coarsest >= 8 expected")
    if not 1 <= iters <= MAX_ITERS or not 0 <= max_shift_q8 <= MAX_SHIFT_Q8 or not 0 <= min_eig < 2 ** 31:
        raise ValueError("iters in 1..16, max_shift_q8 in 0..2048, min_eig >= 0 expected")


def grey(img, rgb_order=0):
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img.astype(np.int64)
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    c = img.astype(np.int64)
    b, r = (c[..., 2], c[..., 0]) if rgb_order else (c[..., 0], c[..., 2])
    return (1868 * b + 9617 * c[..., 1] + 4899 * r + 8192) >> 14


def pyramid(g, coarsest):
    """[level 0 .. coarsest] int64"""
    out = [np.asarray(g, np.int64)]
    for _ in range(coarsest):
        a = out[-1]; h, w = a.shape[0] >> 1, a.shape[1] >> 1
        out.append((a[0:2 * h:2, 0:2 * w:2] + a[0:2 * h:2, 1:2 * w:2] + a[1:2 * h:2, 0:2 * w:2] + a[1:2 * h:2, 1:2 * w:2] + 2) >> 2)
    return out


def origins(n):
    o = list(range(0, n - 7, 4))
    if o[-1] != n - 8:
        o.append(n - 8)
    return np.array(o, np.int64)


def rdiv(a, d):
    """patch_refine_np.rdiv over int64 arrays: a / d to the nearest, halves away from zero; d > 0"""
    m = np.abs(a); q = m // d; r = m - q * d
    q = q + (r >= d - r)
    return np.where(a < 0, -q, q)


def step(num, det):
    """rdiv(-32 num, det) clamped to +-256, without leaving int64: |2 num| = q1 det + r1, then 16 q1 + rdiv(16 r1, det) (16 r1 < 2^60)"""
    m = 2 * np.abs(num); q1 = m // det; r1 = m - q1 * det
    q = np.minimum(16 * np.minimum(q1, 17) + rdiv(16 * r1, det), 256)
    return np.where(num > 0, -q, q)


def sample(G1, X, Y):
    h, w = G1.shape
    X = np.clip(X, 0, (w - 1) * 256); Y = np.clip(Y, 0, (h - 1) * 256)
    ix, fx, iy, fy = X >> 8, X & 255, Y >> 8, Y & 255
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    return (256 - fx) * (256 - fy) * G1[iy, ix] + fx * (256 - fy) * G1[iy, ix1] + (256 - fx) * fy * G1[iy1, ix] + fx * fy * G1[iy1, ix1]


def gradients(G0):
    h, w = G0.shape
    xs, ys = np.arange(w), np.arange(h)
    return G0[:, np.minimum(xs + 1, w - 1)] - G0[:, np.maximum(xs - 1, 0)], G0[np.minimum(ys + 1, h - 1), :] - G0[np.maximum(ys - 1, 0), :]


def initial_field(U_coarser, ys, xs):
    """2 U[l+1][min(y >> 1, h1 - 1)][min(x >> 1, w1 - 1)] at the pixels ys x xs (0 at the coarsest level: U_coarser None)"""
    if U_coarser is None:
        return np.zeros((len(ys), len(xs), 2), np.int64)
    h1, w1 = U_coarser.shape[:2]
    return 2 * U_coarser[np.minimum(ys >> 1, h1 - 1)[:, None], np.minimum(xs >> 1, w1 - 1)[None, :]]


def _note(trace, key, v):
    if trace is not None and np.size(v):
        trace[key] = max(trace.get(key, 0), int(np.abs(v).max()))


def patch_level(G0, G1, U_coarser, iters, max_shift_q8, min_eig, stats, trace=None):
    """The patch flows of one level: (up [ny][nx][2] int64, ys, xs); adds to stats"""
    h, w = G0.shape
    ys, xs = origins(h), origins(w); ny, nx = len(ys), len(xs); P = ny * nx
    u0 = initial_field(U_coarser, ys + 4, xs + 4).reshape(P, 2)
    rr = np.arange(8, dtype=np.int64)
    py = (np.repeat(ys, nx)[:, None, None] + rr[None, :, None]) + np.zeros((1, 1, 8), np.int64)
    px = (np.tile(xs, ny)[:, None, None] + rr[None, None, :]) + np.zeros((1, 8, 1), np.int64)
    GX, GY = gradients(G0)
    T, gx, gy = G0[py, px], GX[py, px], GY[py, px]
    s = lambda a: a.sum(axis=(1, 2))
    sgx, sgy = s(gx), s(gy)
    hxx, hyy, hxy = N * s(gx * gx) - sgx * sgx, N * s(gy * gy) - sgy * sgy, N * s(gx * gy) - sgx * sgy
    det, tr = hxx * hyy - hxy * hxy, hxx + hyy
    _note(trace, "max_h", np.maximum(np.maximum(hxx, hyy), np.abs(hxy))); _note(trace, "max_det", det)
    flat = (det <= 0) | (tr < 2 * min_eig) | (det - min_eig * tr + min_eig * min_eig < 0)

    def evaluate(idx, u):
        S = sample(G1, px[idx] * 256 + u[:, 0, None, None], py[idx] * 256 + u[:, 1, None, None])
        e = (S - 65536 * T[idx] + 2048) >> 12
        se = s(e)
        _note(trace, "max_e", e)
        return N * s(e * e) - se * se, N * s(gx[idx] * e) - sgx[idx] * se, N * s(gy[idx] * e) - sgy[idx] * se

    out = u0.copy()
    act = np.nonzero(~flat)[0]                                            # the patches still iterating
    u = u0[act].copy()
    cost, bx, by = evaluate(act, u)
    best = np.full(P, -1, np.int64); best[act] = cost
    rejected = np.zeros(P, bool); steps = 0
    for _ in range(iters):
        if not len(act):
            break
        numx, numy = hyy[act] * bx - hxy[act] * by, hxx[act] * by - hxy[act] * bx
        _note(trace, "max_b", np.maximum(np.abs(bx), np.abs(by))); _note(trace, "max_2num", 2 * np.maximum(np.abs(numx), np.abs(numy))); _note(trace, "max_cost", cost)
        dx, dy = step(numx, det[act]), step(numy, det[act])
        go = (dx != 0) | (dy != 0)
        act, u, dx, dy = act[go], u[go], dx[go], dy[go]
        u = u + np.stack([dx, dy], 1); steps += len(act)
        left = np.abs(u - u0[act]).max(axis=1) > max_shift_q8 if len(act) else np.zeros(0, bool)
        rejected[act[left]] = True
        act, u = act[~left], u[~left]
        cost, bx, by = evaluate(act, u)
        better = cost < best[act]
        best[act[better]] = cost[better]; out[act[better]] = u[better]
    out[rejected] = u0[rejected]
    stats[0] += int(P - flat.sum() - rejected.sum()); stats[1] += int(flat.sum()); stats[2] += int(rejected.sum()); stats[3] += int(steps)
    return out.reshape(ny, nx, 2), ys, xs


def _containing(o, n):
    """[n][3]: the indices of the origins o whose patch holds the coordinate, -1 = none"""
    t = np.full((n, 3), -1, np.int64); cnt = np.zeros(n, np.int64)
    for j, a in enumerate(o):
        for x in range(int(a), int(a) + 8):
            t[x, cnt[x]] = j; cnt[x] += 1
    return t


def densify(G0, G1, up, ys, xs):
    h, w = G0.shape
    cy, cx = _containing(ys, h), _containing(xs, w)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    sw = np.zeros((h, w), np.int64); sx = np.zeros((h, w), np.int64); sy = np.zeros((h, w), np.int64)
    for a in range(3):
        for b in range(3):
            jy, jx = cy[:, a][:, None] + np.zeros((1, w), np.int64), cx[:, b][None, :] + np.zeros((h, 1), np.int64)
            ok = (jy >= 0) & (jx >= 0)
            u = up[np.maximum(jy, 0), np.maximum(jx, 0)]
            d = np.abs(sample(G1, X * 256 + u[..., 0], Y * 256 + u[..., 1]) - 65536 * G0) >> 16
            wgt = np.where(ok, 65536 // np.maximum(1, d), 0)
            sw += wgt; sx += wgt * u[..., 0]; sy += wgt * u[..., 1]
    return np.stack([rdiv(sx, sw), rdiv(sy, sw)], -1)


def dis_flow(img0, img1, coarsest=4, iters=6, max_shift_q8=1024, min_eig=0, rgb_order=0, trace=None):
    """(flow f32 [h][w][2], q8 i32 [h][w][2], stats i32 [4]): the three outputs of vido_dis_flow.  trace: a dict that collects the largest magnitudes met (max_e, max_b,
    max_h, max_det, max_2num, max_cost)"""
    g0, g1 = grey(img0, rgb_order), grey(img1, rgb_order)
    assert g0.shape == g1.shape
    h, w = g0.shape
    check_params(h, w, coarsest, iters, max_shift_q8, min_eig)
    P0, P1 = pyramid(g0, coarsest), pyramid(g1, coarsest)
    stats = np.zeros(4, np.int64); U = None
    for l in range(coarsest, -1, -1):
        up, ys, xs = patch_level(P0[l], P1[l], U, iters, max_shift_q8, int(min_eig), stats, trace)
        U = densify(P0[l], P1[l], up, ys, xs)
    q8 = U.astype(np.int32)
    return (q8.astype(np.float32) / np.float32(256)), q8, stats.astype(np.int32)


def n_patches(h, w, coarsest):
    return sum(len(origins(h >> l)) * len(origins(w >> l)) for l in range(coarsest + 1))


def resample(img, dx_q8, dy_q8):
    """img seen at (x 256 + dx_q8, y 256 + dy_q8) by the statement's own bilinear form, rounded to bytes: (S + 32768) >> 16"""
    g = np.asarray(img).astype(np.int64); h, w = g.shape
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    return ((sample(g, X * 256 + dx_q8, Y * 256 + dy_q8) + 32768) >> 16).astype(np.uint8)
