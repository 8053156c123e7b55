"""Plain numpy restatement of the tracking front end's data-parallel stages — the second witness beside oracle/track_oracle.c.

Written from the reference lines that csrc/track.hip cites (vido_slam/src), not from the C oracle:
  Tracking.cc:299-322   depth pre-scale          Frame.cc:72-100, 165-177  static candidates
  Frame.cc:184-211      dense object samples     Tracking.cc:369-391 / 398-421  hand-over gathers
  Tracking.cc:3291-3357 UpdateMask               Frame.cc:706-771  back-projection   Tracking.cc:1582-1668  scene flow
float32 wherever the reference computes in float; float64 for the accumulation of the cv::Mat products (`Rwl*x3Dc`, `-Rlw.t()*tlw`), whose result
is rounded to float before the float addition of twl — the convention of include/vido_slam/cv_compat.h.  `int x = pt.x` is C's truncation towards
zero: astype(int32) on finite values inside the int range, which is all a caller may pass (the conversion of NaN is undefined in C)."""
import numpy as np

F = np.float32


def _trunc(a):
    return np.asarray(a, F).astype(np.int32)


def depth_prescale(depth, mode, factor, bf, scale):
    """Tracking.cc:299-322: d < 0 -> 0, else OMD d/f, KITTI bf/(d/f), KAIST scale*bf/(d/f)."""
    d = np.asarray(depth, F)
    factor, bf, scale = F(factor), F(bf), F(scale)
    with np.errstate(all="ignore"):
        q = d / factor
        r = q if mode == 0 else bf / q if mode == 1 else (scale * bf) / q
    return np.where(d < 0, F(0), r).astype(F)


def static_candidates(kps, depth, flow, mask, th_depth):
    """Frame.cc:72-100 + 165-177 -> (index into kps, correspondence, flow, depth or -1)."""
    h, w = depth.shape
    kx, ky = np.asarray(kps["x"], F), np.asarray(kps["y"], F)
    x, y = _trunc(kx), _trunc(ky)
    d = depth[y, x]
    fx, fy = flow[y, x, 0], flow[y, x, 1]
    with np.errstate(invalid="ignore"):
        ok = (mask[y, x] == 0) & ~((d > F(th_depth)) | (d <= 0))
        ok &= (fx != 0) & (fy != 0)
        ok &= (kx + fx < F(w)) & (ky + fy < F(h)) & (kx < F(w)) & (ky < F(h))
        i = np.nonzero(ok)[0].astype(np.int32)
        corr = np.stack([kx[i] + fx[i], ky[i] + fy[i]], 1).astype(F)
        dd = np.where(d[i] > 0, d[i], F(-1)).astype(F)
    return i, corr, np.stack([fx[i], fy[i]], 1).astype(F), dd


def dense_object_samples(depth, flow, mask, th_obj, step=4):
    """Frame.cc:184-211, lattice visited row-major -> (keys, correspondence, depth, label, flow)."""
    h, w = depth.shape
    ii, jj = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    d, m = depth[ii, jj], mask[ii, jj]
    fx, fy = flow[ii, jj, 0], flow[ii, jj, 1]
    jf, jif = jj.astype(F), ii.astype(F)
    with np.errstate(invalid="ignore"):
        ok = (m != 0) & (d < F(th_obj)) & (d > 0)
        ok &= (jf + fx < F(w)) & (jf + fx > 0) & (jif + fy < F(h)) & (jif + fy > 0)
    s = np.nonzero(ok)[0]
    return (np.stack([jf[s], jif[s]], 1), np.stack([jf[s] + fx[s], jif[s] + fy[s]], 1).astype(F), d[s].astype(F), m[s].astype(np.int32),
            np.stack([fx[s], fy[s]], 1).astype(F))


def _strictly_inside_minus_one(u, v, w, h):
    return (u < w - 1) & (u > 0) & (v < h - 1) & (v > 0)


def gather_static_depth(keys, depth):
    """Tracking.cc:369-391."""
    keys = np.asarray(keys, F).reshape(-1, 2); h, w = depth.shape
    u, v = _trunc(keys[:, 0]), _trunc(keys[:, 1])
    ins = _strictly_inside_minus_one(u, v, w, h)
    d = depth[np.where(ins, v, 0), np.where(ins, u, 0)]
    with np.errstate(invalid="ignore"):
        return np.where(ins & (d > 0), d, F(-1)).astype(F)


def gather_object_depth_label(keys, depth, mask, th_obj):
    """Tracking.cc:398-421."""
    keys = np.asarray(keys, F).reshape(-1, 2); h, w = depth.shape
    u, v = _trunc(keys[:, 0]), _trunc(keys[:, 1])
    ins = _strictly_inside_minus_one(u, v, w, h)
    vv, uu = np.where(ins, v, 0), np.where(ins, u, 0)
    d = depth[vv, uu]
    with np.errstate(invalid="ignore"):
        ok = ins & (d < F(th_obj)) & (d > 0)
    return np.where(ok, d, F(0.1)).astype(F), np.where(ok, mask[vv, uu], 0).astype(np.int32)


def point_samples(xy, depth, flow, mask):
    """The map reads of Tracking::RenewFrameInfo at a point list.  THE RULE: a point whose truncated position lies inside [0,w) x [0,h) gives
    the map values there; any other point gives zeros.  -> (mask, depth, flow)."""
    xy = np.asarray(xy, F).reshape(-1, 2); h, w = depth.shape
    u, v = _trunc(xy[:, 0]), _trunc(xy[:, 1])
    ins = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    vv, uu = np.where(ins, v, 0), np.where(ins, u, 0)
    return (np.where(ins, mask[vv, uu], 0).astype(np.int32), np.where(ins, depth[vv, uu], F(0)).astype(F),
            np.where(ins[:, None], flow[vv, uu], F(0)).astype(F))


def update_mask(last_label, last_corr, mask_last, flow_last, mask_cur):
    """Tracking.cc:3291-3357, one label after the other in ascending order: a label votes on the mask as the labels before it left it.
    The most frequent value is sorted[0] after std::sort by descending count of (value, count) pairs taken from a std::map, i.e. in ascending value;
    for the handful of distinct values of a vote that sort is an insertion sort, which keeps equal counts in map order: the smallest value wins a tie.
    -> (patched mask, recovered labels)."""
    last_label = np.asarray(last_label, np.int32); last_corr = np.asarray(last_corr, F).reshape(-1, 2)
    out = np.array(mask_cur, np.int32, copy=True); h, w = out.shape
    rec = []
    for lab in np.unique(last_label):
        c = last_corr[last_label == lab]
        u, v = _trunc(c[:, 0]), _trunc(c[:, 1])
        ins = (u < w) & (u > 0) & (v < h) & (v > 0)
        votes = out[v[ins], u[ins]]
        if len(votes) < 100:
            continue
        vals, cnt = np.unique(votes, return_counts=True)
        if vals[np.argsort(-cnt, kind="stable")[0]] != 0:
            continue
        j, k = np.nonzero(mask_last == lab)
        fx, fy = _trunc(flow_last[j, k, 0]), _trunc(flow_last[j, k, 1])
        ok = (k + fx < w) & (k + fx > 0) & (j + fy < h) & (j + fy > 0)
        out[(j + fy)[ok], (k + fx)[ok]] = lab
        rec.append(int(lab))
    return out, np.array(rec, np.int32)


def unproject_world(keys, z, fx, fy, cx, cy, Tcw):
    """Frame.cc:706-771 with addnoise = 0; z not > 0 gives no point (zeros here)."""
    keys = np.asarray(keys, F).reshape(-1, 2); z = np.asarray(z, F); Tcw = np.asarray(Tcw, F)
    invfx, invfy = F(1) / F(fx), F(1) / F(fy)
    Rwl = Tcw[:3, :3].T.astype(np.float64); tlw = Tcw[:3, 3].astype(np.float64)
    twl = (((-Rwl[:, 0]) * tlw[0] + (-Rwl[:, 1]) * tlw[1]) + (-Rwl[:, 2]) * tlw[2]).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((keys[:, 0] - F(cx)) * z * invfx).astype(np.float64); y = ((keys[:, 1] - F(cy)) * z * invfy).astype(np.float64)
        zz = z.astype(np.float64)
        out = np.empty((len(z), 3), F)
        for r in range(3):
            s = (Rwl[r, 0] * x + Rwl[r, 1] * y) + Rwl[r, 2] * zz
            out[:, r] = s.astype(F) + twl[r]
        out[~(z > 0)] = 0
    return out


def scene_flow(xl, xc, sl, sc, obj_label):
    """Tracking.cc:1582-1668: X_w(cur) - X_w(last) where both semantic labels are > 0; otherwise object label -1 and no flow."""
    xl = np.asarray(xl, F); xc = np.asarray(xc, F); sl = np.asarray(sl, np.int32); sc = np.asarray(sc, np.int32)
    bad = (sc <= 0) | (sl <= 0)
    with np.errstate(invalid="ignore", over="ignore"):
        f3 = np.where(bad[:, None], F(0), xc - xl).astype(F)
    return f3, np.where(bad, -1, np.asarray(obj_label, np.int32)).astype(np.int32)
