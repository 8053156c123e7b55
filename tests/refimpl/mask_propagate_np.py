"""Label-image propagation through dense flow, stated in plain numpy: the reference of vido_mask_propagate / vido_frame_propagate_mask (include/vido_c.h).

propagate(mask_prev, flow, depth_prev=None) -> (out int32 [H,W], stats int32 [3] = sources kept, pixels hit, pixels filled)

  1. a source is a pixel with label L > 0 whose flow components are both finite with |f| < 32768 and, with a depth map, whose depth is finite and > 0; its target is
     (x + rint(dx), y + rint(dy)) (np.rint on float32: nearest, ties to even), kept iff inside the image;
  2. a target takes the minimum over its sources of (depth bits as u32) << 32 | (u32)L  (upper half 0 without depth);
  3. an unhit target takes L iff at least 5 of its 8 neighbours were hit and resolved to L in step 2 (outside the image = not hit); one pass; everything else is 0.
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def scatter_keys(mask_prev, flow, depth_prev=None):
    """Step 1 + 2: the u64 key plane (EMPTY where nothing landed) and the number of sources kept."""
    mask_prev = np.asarray(mask_prev); flow = np.asarray(flow)
    assert mask_prev.dtype == np.int32 and mask_prev.ndim == 2 and flow.dtype == np.float32 and flow.shape == mask_prev.shape + (2,)
    H, W = mask_prev.shape
    fx, fy = flow[..., 0], flow[..., 1]
    with np.errstate(invalid="ignore"):
        src = (mask_prev > 0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < np.float32(32768)) & (np.abs(fy) < np.float32(32768))
        if depth_prev is not None:
            depth_prev = np.asarray(depth_prev)
            assert depth_prev.dtype == np.float32 and depth_prev.shape == (H, W)
            src &= np.isfinite(depth_prev) & (depth_prev > 0)
    ys, xs = np.nonzero(src)
    tx = xs.astype(np.int64) + np.rint(fx[ys, xs]).astype(np.int64)
    ty = ys.astype(np.int64) + np.rint(fy[ys, xs]).astype(np.int64)
    keep = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    ys, xs, tx, ty = ys[keep], xs[keep], tx[keep], ty[keep]
    key = mask_prev[ys, xs].astype(np.uint32).astype(np.uint64)
    if depth_prev is not None:
        key |= np.ascontiguousarray(depth_prev[ys, xs]).view(np.uint32).astype(np.uint64) << np.uint64(32)
    plane = np.full(H * W, EMPTY, np.uint64)
    np.minimum.at(plane, ty * W + tx, key)
    return plane.reshape(H, W), int(keep.sum())


def propagate(mask_prev, flow, depth_prev=None, votes=5):
    plane, n_src = scatter_keys(mask_prev, flow, depth_prev)
    H, W = plane.shape
    hit = plane != EMPTY
    lab = np.where(hit, (plane & np.uint64(0xFFFFFFFF)).astype(np.int64), 0).astype(np.int32)      # a source's label is > 0: 0 can stand for "not hit"
    pad = np.zeros((H + 2, W + 2), np.int32); pad[1:-1, 1:-1] = lab
    nb = np.stack([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)])      # [8,H,W], 0 = not hit
    fill = np.zeros((H, W), np.int32)
    for k in range(8):                                                   # a label with >= 5 of 8 votes is unique (votes >= 5); with fewer votes asked the first in neighbour order wins
        cand = nb[k]
        cnt = (nb == cand[None]).sum(0)
        fill = np.where((fill == 0) & (cand > 0) & (cnt >= votes), cand, fill)
    out = np.where(hit, lab, fill).astype(np.int32)
    n_fill = int(((~hit) & (fill != 0)).sum())
    return out, np.array([n_src, int(hit.sum()), n_fill], np.int32)
