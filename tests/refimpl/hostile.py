"""Hostile inputs for the front-end list kernels (tests only): maps and keypoints built to sit ON the branches of Frame.cc:72-211 and
Tracking.cc:299-421, 3291-3357, plus the census that proves a seed really put them there.

Stated proportions (of all pixels, drawn independently of position):
  flow, 3 % each  — leaves the image on the left / right / top / bottom; fx exactly 0.0; fy exactly 0.0; both 0.0; NaN (fx, fy or both); and 5 % each
                    (they only count at integer probe positions) — lands exactly on x = w, y = h, x = 0, y = 0.  NaN flow never reaches a float -> int conversion in these stages: a probe carrying it fails every
                    comparison and is dropped, and UpdateMask's scenes (um_*_scene below) keep NaN outside the scattered labels.
  depth, 4 % each — equal to the threshold that applies to the pixel (ThDepthObj under a label, ThDepthBG elsewhere), nextafter above it, nextafter
                    below it, 0, negative (the pre-scale turns it into 0), NaN.
Labels form a frame along all four image borders (so lattice row 0, column 0, the last lattice row and the last lattice column carry labels) and a block in
the centre.  Keypoints: 20 at (w-1, h-1), 20 at (0, 0), a quarter just below an integer in both coordinates, a quarter at integer positions (only
there can `x + fx` hit w exactly), a tenth on the last row / last column, the rest anywhere."""
import functools
import numpy as np
from . import track_np

F = np.float32
TH_BG, TH_OBJ = 40.0, 25.0
P_FLOW_CASES = [0.03] * 4 + [0.05] * 4 + [0.03] * 4      # left, right, top, bottom | on w, on h, on x 0, on y 0 | fx 0, fy 0, both 0, NaN
P_DEPTH = 0.04
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
SIZES = [(1242, 375), (1241, 376), (1280, 560), (640, 192), (201, 151)]      # the last: a small odd size (odd pixel count) the context accepts


def maps(seed, w, h):
    """-> raw depth (h,w) f32 (before the pre-scale; dataset 0 with factor 1 leaves all but the negatives as they are), flow (h,w,2) f32, mask (h,w) i32."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    xf, yf = xx.astype(F), yy.astype(F)
    depth = rng.uniform(1, 50, (h, w)).astype(F)
    flow = (rng.uniform(0.25, 6, (h, w, 2)) * rng.choice([-1.0, 1.0], (h, w, 2))).astype(F)
    mask = np.zeros((h, w), np.int32)
    b = max(8, min(w, h) // 8)
    mask[:b, :] = 1; mask[:, :b] = 2; mask[h - b:, :] = 3; mask[:, w - b:] = 4
    mask[h // 3:2 * h // 3, w // 3:2 * w // 3] = 5
    k = np.searchsorted(np.cumsum(P_FLOW_CASES), rng.random_sample((h, w)), side="right")       # 0..11: the case, 12: none
    off = rng.uniform(0.5, 30, (h, w)).astype(F)
    fx, fy = flow[..., 0], flow[..., 1]
    fx[k == 0] = (-xf - off)[k == 0]; fx[k == 1] = ((F(w) - xf) + off)[k == 1]
    fy[k == 2] = (-yf - off)[k == 2]; fy[k == 3] = ((F(h) - yf) + off)[k == 3]
    fx[k == 4] = (F(w) - xf)[k == 4]; fy[k == 5] = (F(h) - yf)[k == 5]
    fx[k == 6] = (-xf)[k == 6]; fy[k == 7] = (-yf)[k == 7]
    fx[(k == 8) | (k == 10)] = 0; fy[(k == 9) | (k == 10)] = 0
    which = rng.randint(0, 3, (h, w))
    fx[(k == 11) & (which != 1)] = np.nan; fy[(k == 11) & (which != 0)] = np.nan
    kd = np.floor(rng.random_sample((h, w)) / P_DEPTH).astype(int)
    th = np.where(mask != 0, F(TH_OBJ), F(TH_BG)).astype(F)
    depth[kd == 0] = th[kd == 0]
    depth[kd == 1] = np.nextafter(th, F(np.inf))[kd == 1]; depth[kd == 2] = np.nextafter(th, F(-np.inf))[kd == 2]
    depth[kd == 3] = 0; depth[kd == 4] = -rng.uniform(0.5, 5, (h, w)).astype(F)[kd == 4]; depth[kd == 5] = np.nan
    # the two corner keypoints of the issue sit on benign, unlabelled pixels so that they survive
    for (y, x, f) in ((0, 0, (1.5, 2.5)), (h - 1, w - 1, (-1.5, -2.5))):
        mask[y, x] = 0; depth[y, x] = 10; flow[y, x] = f
    return depth, flow, mask


def keypoints(seed, w, h, n):
    rng = np.random.RandomState(seed + 7919)
    lim_x, lim_y = np.nextafter(F(w), F(0)), np.nextafter(F(h), F(0))
    x = np.minimum(rng.uniform(0, w, n).astype(F), lim_x); y = np.minimum(rng.uniform(0, h, n).astype(F), lim_y)
    kind = rng.random_sample(n)
    below = kind < 0.25
    x[below] = np.nextafter(rng.randint(1, w, n).astype(F), F(0))[below]; y[below] = np.nextafter(rng.randint(1, h, n).astype(F), F(0))[below]
    integer = (kind >= 0.25) & (kind < 0.5)
    x[integer] = np.floor(x[integer]); y[integer] = np.floor(y[integer])
    y[(kind >= 0.5) & (kind < 0.55)] = np.minimum(F(h - 1) + rng.random_sample(n).astype(F), lim_y)[(kind >= 0.5) & (kind < 0.55)]
    x[(kind >= 0.55) & (kind < 0.6)] = np.minimum(F(w - 1) + rng.random_sample(n).astype(F), lim_x)[(kind >= 0.55) & (kind < 0.6)]
    fixed = rng.permutation(n)[:40]
    x[fixed[:20]] = w - 1; y[fixed[:20]] = h - 1; x[fixed[20:]] = 0; y[fixed[20:]] = 0
    assert (x.astype(np.int32) >= 0).all() and (x.astype(np.int32) < w).all() and (y.astype(np.int32) >= 0).all() and (y.astype(np.int32) < h).all()
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"] = x, y, 31.0, rng.uniform(0, 360, n), rng.uniform(1, 100, n), rng.randint(0, 8, n)
    return k


@functools.lru_cache(maxsize=64)
def frame(seed, w, h, n_kp):
    """One generated frame, cached: (raw depth, flow, mask, keypoints).  Callers copy what they mutate."""
    d, f, m = maps(seed, w, h)
    for a in (d, f, m):
        a.setflags(write=False)
    return d, f, m, keypoints(seed, w, h, n_kp)


def census(depth_raw, flow, mask, kps):
    """How often each hostile case occurs where it matters, classified with the numpy reference's own arithmetic (float32, C truncation):
    flow cases at the probes that REACH the flow test (keypoints on unlabelled pixels with usable depth; labelled lattice probes with usable depth),
    depth cases at every keypoint pixel without a label (against ThDepthBG) and every labelled lattice probe (against ThDepthObj)."""
    h, w = mask.shape
    depth = track_np.depth_prescale(depth_raw, 0, 1.0, 1.0, 1.0)
    c = {}
    kx, ky = kps["x"], kps["y"]; x, y = kx.astype(np.int32), ky.astype(np.int32)
    ii, jj = [a.ravel() for a in np.meshgrid(np.arange(0, h, 4), np.arange(0, w, 4), indexing="ij")]
    with np.errstate(invalid="ignore"):
        ds, do = depth[y, x], depth[ii, jj]
        reach_s = (mask[y, x] == 0) & ~((ds > F(TH_BG)) | (ds <= 0))
        reach_o = (mask[ii, jj] != 0) & (do < F(TH_OBJ)) & (do > 0)
        px = np.concatenate([kx[reach_s], jj[reach_o].astype(F)]); py = np.concatenate([ky[reach_s], ii[reach_o].astype(F)])
        fx = np.concatenate([flow[y, x, 0][reach_s], flow[ii, jj, 0][reach_o]]); fy = np.concatenate([flow[y, x, 1][reach_s], flow[ii, jj, 1][reach_o]])
        c["flow_left"] = (px + fx < 0).sum(); c["flow_right"] = (px + fx > F(w)).sum(); c["flow_top"] = (py + fy < 0).sum(); c["flow_bottom"] = (py + fy > F(h)).sum()
        c["flow_on_w"] = (px + fx == F(w)).sum(); c["flow_on_h"] = (py + fy == F(h)).sum()
        c["flow_on_x0"] = ((px + fx == 0) & (fx != 0)).sum(); c["flow_on_y0"] = ((py + fy == 0) & (fy != 0)).sum()
        c["flow_fx0"] = ((fx == 0) & (fy != 0)).sum(); c["flow_fy0"] = ((fy == 0) & (fx != 0)).sum(); c["flow_both0"] = ((fx == 0) & (fy == 0)).sum()
        c["flow_nan"] = (np.isnan(fx) | np.isnan(fy)).sum()
        for name, sel_d, raw, th in (("bg", ds[mask[y, x] == 0], depth_raw[y, x][mask[y, x] == 0], F(TH_BG)),
                                     ("obj", do[mask[ii, jj] != 0], depth_raw[ii, jj][mask[ii, jj] != 0], F(TH_OBJ))):
            c[name + "_depth_eq"] = (sel_d == th).sum(); c[name + "_depth_above"] = (sel_d == np.nextafter(th, F(np.inf))).sum()
            c[name + "_depth_below"] = (sel_d == np.nextafter(th, F(-np.inf))).sum()
            c[name + "_depth_zero"] = (raw == 0).sum(); c[name + "_depth_neg"] = (raw < 0).sum(); c[name + "_depth_nan"] = np.isnan(raw).sum()
    lab = mask[ii, jj] != 0
    c["label_row0"] = (lab & (ii == 0)).sum(); c["label_col0"] = (lab & (jj == 0)).sum()
    c["label_last_row"] = (lab & (ii == ii.max())).sum(); c["label_last_col"] = (lab & (jj == jj.max())).sum()
    c["kp_last_pixel"] = ((kx == w - 1) & (ky == h - 1)).sum(); c["kp_origin"] = ((kx == 0) & (ky == 0)).sum()
    c["kp_below_integer"] = ((np.nextafter(kx, F(np.inf)) == np.ceil(kx)) & (kx != np.ceil(kx)) & (np.nextafter(ky, F(np.inf)) == np.ceil(ky)) & (ky != np.ceil(ky))).sum()
    c["kp_last_row"] = (y == h - 1).sum(); c["kp_last_col"] = (x == w - 1).sum()
    return {k: int(v) for k, v in c.items()}


@functools.lru_cache(maxsize=64)
def check_hostile(seed, w, h, n_kp):
    """Asserts that frame(seed, w, h, n_kp) holds every case at least 20 times and leaves non-trivial lists; -> the census."""
    d, f, m, kps = frame(seed, w, h, n_kp)
    c = census(d, f, m, kps)
    thin = {k: v for k, v in c.items() if v < 20}
    assert not thin, ("hostile cases missing from seed %d at %dx%d" % (seed, w, h), thin)
    ds = track_np.depth_prescale(d, 0, 1.0, 1.0, 1.0)
    n_stat = len(track_np.static_candidates(kps, ds, f, m, TH_BG)[0]); n_obj = len(track_np.dense_object_samples(ds, f, m, TH_OBJ)[0])
    assert n_stat >= 50 and n_obj >= 100, (n_stat, n_obj)
    return c


# ---- UpdateMask scenes ------------------------------------------------------------------------------------
def _block(a, x0, y0, s, v):
    a[y0:y0 + s, x0:x0 + s] = v


def um_sequential_scene(w, h):
    """Five 48 x 48 objects in the last frame (144 lattice samples each), every size >= 201 x 151.  The detector lost labels 1, 2, 3 and 5 in the current frame.
      1 (A): votes 0 -> recovered; its scatter (integer flow (2, 3)) fills [10,58) x [11,59).
      2 (B): 110 of its 144 propagated samples fall into that rectangle: BEFORE A's scatter its vote is 0, AFTER it the vote is 1 -> not recovered.
      3 (C): votes 0 -> recovered in a later round; scatter fills [123,171) x [6,54).
      4    : still detected where it moved to -> votes 4, not recovered.
      5 (E): all 144 samples fall into C's rectangle -> votes 3 after C's scatter (0 before) -> not recovered.
    Sequential answer [1, 3]; a vote on the unpatched mask would give [1, 2, 3, 5].  Flow outside the objects is NaN: UpdateMask must not convert it.
    -> dict(depth, flow_last, mask_last, mask_cur, th_obj)"""
    assert w >= 201 and h >= 151
    mask_last = np.zeros((h, w), np.int32); flow = np.full((h, w, 2), np.nan, F)
    for lab, x0, y0, f in ((1, 8, 8, (2.5, 3.5)), (2, 64, 8, (-44.25, 1.75)), (3, 120, 8, (3.25, -2.5)), (4, 8, 64, (1.5, 1.5)), (5, 64, 64, (60.5, -56.25))):
        _block(mask_last, x0, y0, 48, lab); flow[y0:y0 + 48, x0:x0 + 48] = f
    mask_cur = np.zeros((h, w), np.int32); _block(mask_cur, 9, 65, 48, 4)
    return dict(depth=np.full((h, w), 10, F), flow_last=flow, mask_last=mask_last, mask_cur=mask_cur)


def um_edge_scene(w, h):
    """Hand-built sample lists (UpdateMask takes lists; they need not come from the sampler).  Current mask: 0 except a patch of label 6.
      7 : exactly 100 samples, all in the image, on 0           -> recovered
      8 : 100 samples, one at u = 0 (not `> 0`): 99 in the image -> skipped although its vote would be 0
      9 : 100 samples, 50 on 0 and 50 on label 6: a tie          -> the smaller value, 0, wins -> recovered
      10: object in the bottom-right corner, flow (+12, +12): row h-13 / column w-13 land exactly on h-1 / w-1 (written), everything after them leaves the image
      11: object in the top-left corner, flow (-12, -12): targets at 0 are refused (`> 0`), targets at 1 are written
    -> dict(mask_last, flow_last, mask_cur, last_label, last_corr); expected recovered [7, 9, 10, 11]."""
    mask_last = np.zeros((h, w), np.int32); flow = np.full((h, w, 2), np.nan, F)
    _block(mask_last, 60, 60, 24, 7); flow[60:84, 60:84] = (5.5, -4.5)
    _block(mask_last, 100, 60, 24, 8); flow[60:84, 100:124] = (-3.5, 2.5)
    _block(mask_last, 140, 60, 24, 9); flow[60:84, 140:164] = (1.25, 1.75)
    mask_last[h - 30:, w - 30:] = 10; flow[h - 30:, w - 30:] = (12.0, 12.0)
    mask_last[:30, :30] = 11; flow[:30, :30] = (-12.0, -12.0)
    mask_cur = np.zeros((h, w), np.int32); mask_cur[100:120, 20:120] = 6
    lab, corr = [], []
    def add(label, pts):
        lab.extend([label] * len(pts)); corr.extend(pts)
    add(7, [(30.25 + i, 90.5) for i in range(100)])
    add(8, [(0.5, 91.5)] + [(30.25 + i, 91.5) for i in range(99)])
    add(9, [(25.5 + i, 105.5) for i in range(50)] + [(25.5 + i, 95.5) for i in range(50)])
    add(10, [(30.75 + i, 92.5) for i in range(100)])
    add(11, [(30.75 + i, 93.5) for i in range(120)])
    order = np.random.RandomState(5).permutation(len(lab))                               # the lists are not grouped by label
    return dict(mask_last=mask_last, flow_last=flow, mask_cur=mask_cur, last_label=np.array(lab, np.int32)[order], last_corr=np.array(corr, F)[order])


def points_scene(seed, n, w, h):
    """Inputs of back-projection and scene flow: z of 0, negative and NaN among ordinary depths, a pose with a translation of 1e4, semantic labels of 0 and below."""
    rng = np.random.RandomState(seed)
    keys = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(F)
    z = rng.uniform(0.5, 60, n).astype(F)
    kind = rng.randint(0, 10, n)
    z[kind == 0] = 0; z[kind == 1] = -rng.uniform(0.1, 9, n).astype(F)[kind == 1]; z[kind == 2] = np.nan
    a, b = 0.3, -0.2
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Tcw = np.eye(4); Tcw[:3, :3] = Ry @ Rx; Tcw[:3, 3] = (1e4, -7321.5, 1234.25)
    sem_last = rng.randint(1, 6, n).astype(np.int32); sem_cur = sem_last.copy()
    sem_last[rng.randint(0, 8, n) == 0] = 0; sem_cur[rng.randint(0, 8, n) == 0] = -1; sem_cur[rng.randint(0, 8, n) == 1] = 0; sem_last[rng.randint(0, 16, n) == 1] = -3
    return dict(keys=keys, z=z, Tcw=Tcw.astype(F), sem_last=sem_last, sem_cur=sem_cur, obj_label=rng.randint(-2, 9, n).astype(np.int32))
