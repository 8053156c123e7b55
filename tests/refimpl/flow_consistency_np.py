"""The statement of vido_flow_consistency in numpy int64 (no GPU; no float apart from the marked output): the forward-backward check of two dense flow fields in 1/256 px.
csrc/flowcheck.hip must equal every output bit for bit.

Inputs: fwd, bwd int32 [H][W][2] (dx, dy) in 1/256 px — the flow of image 0 -> 1 on image 0's grid and of image 1 -> 0 on image 1's grid, the layout of vido_dis_flow's q8;
1 <= H, W <= 4095; alpha_q10 in 0..1024 (alpha = alpha_q10 / 1024), beta_q16 in 0..2^30 (beta = beta_q16 / 65536 px^2, held in (1/256 px)^2).  For pixel (x, y) with
f = fwd[y][x], in the order the rules apply:
    status 3     not a flow: |f.x| >= 2^19 or |f.y| >= 2^19
    status 2     leaves the image: tx = 256 x + f.x, ty = 256 y + f.y; tx < 0 or tx > 256 (W - 1) or ty < 0 or ty > 256 (H - 1)
    taps         x0 = tx >> 8, ax = tx & 255, x1 = min(x0 + 1, W - 1), y likewise; the four taps bwd[y0][x0], bwd[y0][x1], bwd[y1][x0], bwd[y1][x1] (all four, also where
                 a weight is 0); status 3 when a component of one of them has |.| >= 2^19
    b            s = (256 - ax)(256 - ay) B[y0][x0] + ax (256 - ay) B[y0][x1] + (256 - ax) ay B[y1][x0] + ax ay B[y1][x1] per component (weights sum 65536: |s| < 2^35),
                 b = (s + 32768) >> 16, arithmetic shift (floor): |b| < 2^19
    r            r = f + b, |r.x|, |r.y| < 2^20
    status 1     inconsistent: 1024 |r|^2 > alpha_q10 (|f|^2 + |b|^2) + 1024 beta_q16, squares summed over both components; else status 0
Outputs: status u8 [H][W]; flow_marked f32 [H][W][2] = f / 256 (exact: |f| < 2^19) where the status is 0, elsewhere the quiet NaN with bits 0x7FC00000 on both components;
stats int32 [4] = the count of each status.

Bounds (all arithmetic fits int64): |r|^2 < 2^41, 1024 |r|^2 < 2^51; |f|^2 + |b|^2 < 2^40, times alpha_q10 <= 2^10: < 2^50; 1024 beta_q16 <= 2^40; the right side < 2^51:
every term stays below 2^52."""
import numpy as np

LIMIT = 1 << 19                                    # a component at or past it is not a flow
MAX_SIZE = 4095
MAX_ALPHA_Q10 = 1024
MAX_BETA_Q16 = 1 << 30
DEFAULTS = dict(alpha_q10=10, beta_q16=32768)      # alpha = 0.01, beta = 0.5 px^2 (tools/measure_flow_consistency.py)
NAN_BITS = 0x7FC00000


def check_params(h, w, alpha_q10, beta_q16):
    if not (1 <= w <= MAX_SIZE and 1 <= h <= MAX_SIZE):
        raise ValueError("1 <= w, h <= 4095 expected")
    if not 0 <= alpha_q10 <= MAX_ALPHA_Q10 or not 0 <= beta_q16 <= MAX_BETA_Q16:
        raise ValueError("alpha_q10 in 0..1024, beta_q16 in 0..2^30 expected")


def backward_at_target(fwd, bwd):
    """(b int64 [H][W][2], status int64 [H][W] in {0, 2, 3}): the backward flow sampled at every pixel's target, 0 where the status is not 0"""
    f = np.asarray(fwd).astype(np.int64); B = np.asarray(bwd).astype(np.int64)
    h, w = f.shape[:2]
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    status = np.zeros((h, w), np.int64)
    bad_f = (np.abs(f) >= LIMIT).any(-1)
    tx, ty = 256 * X + f[..., 0], 256 * Y + f[..., 1]
    out = (tx < 0) | (tx > 256 * (w - 1)) | (ty < 0) | (ty > 256 * (h - 1))
    status[out] = 2
    status[bad_f] = 3
    ok = status == 0
    tx, ty = np.where(ok, tx, 0), np.where(ok, ty, 0)
    x0, ax, y0, ay = tx >> 8, tx & 255, ty >> 8, ty & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    t00, t01, t10, t11 = B[y0, x0], B[y0, x1], B[y1, x0], B[y1, x1]
    bad_t = ok & ((np.abs(t00) >= LIMIT) | (np.abs(t01) >= LIMIT) | (np.abs(t10) >= LIMIT) | (np.abs(t11) >= LIMIT)).any(-1)
    status[bad_t] = 3
    ax, ay = ax[..., None], ay[..., None]
    s = (256 - ax) * (256 - ay) * t00 + ax * (256 - ay) * t01 + (256 - ax) * ay * t10 + ax * ay * t11
    b = (s + 32768) >> 16
    b[status != 0] = 0
    return b, status


def flow_consistency(fwd, bwd, alpha_q10=DEFAULTS["alpha_q10"], beta_q16=DEFAULTS["beta_q16"]):
    """(status u8 [H][W], flow_marked f32 [H][W][2], stats i32 [4]): the three outputs of vido_flow_consistency"""
    fwd, bwd = np.asarray(fwd), np.asarray(bwd)
    assert fwd.dtype == np.int32 and bwd.dtype == np.int32 and fwd.ndim == 3 and fwd.shape[2] == 2 and fwd.shape == bwd.shape
    h, w = fwd.shape[:2]
    check_params(h, w, alpha_q10, beta_q16)
    f = fwd.astype(np.int64)
    b, status = backward_at_target(fwd, bwd)
    fz = np.where((status == 0)[..., None], f, 0)
    r = fz + b
    lhs = 1024 * (r * r).sum(-1)
    rhs = np.int64(alpha_q10) * ((fz * fz).sum(-1) + (b * b).sum(-1)) + 1024 * np.int64(beta_q16)
    status[(status == 0) & (lhs > rhs)] = 1
    marked = np.full((h, w, 2), NAN_BITS, np.uint32).view(np.float32)
    keep = status == 0
    marked[keep] = f[keep].astype(np.float32) / np.float32(256)
    stats = np.array([(status == k).sum() for k in range(4)], np.int32)
    return status.astype(np.uint8), marked, stats
