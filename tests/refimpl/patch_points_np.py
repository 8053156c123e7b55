"""The statement of vido_orb_patch_points in numpy and Python integers (no GPU, no float): the 8 x 8 patch at caller-given points of a pyramid level, its three
integer correlation sums against a reference patch, and the verdict.  csrc/patchpts.hip must equal every output bit for bit.

Point k = (x, y, level) in level coordinates.  The patch is rows y-4 .. y+3, columns x-4 .. x+3 of that level, row-major (64 bytes).  A point whose level is out of range or
whose patch is not wholly inside the level is invalid: status -1, sums 0 0 0, zero patch.  With a = reference patch, b = the level's patch:
    S1 = sum a, S2 = sum b, S11 = sum a^2, S22 = sum b^2, S12 = sum a b
    var_ref = 64 S11 - S1^2, var_cur = 64 S22 - S2^2, cov = 64 S12 - S1 S2                      (sums = cov, var_ref, var_cur)
    status 2  if var_ref < min_var or var_cur < min_var                                          (no texture: no evidence)
    status 0  iff cov > 0 and cov^2 * 1024^2 >= min_zncc_q10^2 * var_ref * var_cur               (accepted; exact integers, equality accepts)
    status 1  otherwise                                                                          (rejected)
ZNCC = cov / sqrt(var_ref var_cur), so status 0 is ZNCC >= min_zncc_q10 / 1024 for a positive covariance."""
import numpy as np

VAR_MAX = 66585600            # a 0 / 255 checkerboard: 64 * 32 * 255^2 - (32 * 255)^2


def sums(a, b):
    """(cov, var_ref, var_cur) of two 64-byte patches, as Python integers"""
    a = [int(v) for v in np.asarray(a, np.uint8).reshape(64)]; b = [int(v) for v in np.asarray(b, np.uint8).reshape(64)]
    s1, s2 = sum(a), sum(b)
    s11 = sum(v * v for v in a); s22 = sum(v * v for v in b); s12 = sum(u * v for u, v in zip(a, b))
    return 64 * s12 - s1 * s2, 64 * s11 - s1 * s1, 64 * s22 - s2 * s2


def verdict(cov, var_ref, var_cur, min_var, min_zncc_q10):
    if min_var < 0 or not 0 <= min_zncc_q10 <= 1024:
        raise ValueError("min_var >= 0 and 0 <= min_zncc_q10 <= 1024 expected")
    if var_ref < min_var or var_cur < min_var:
        return 2
    if cov > 0 and cov * cov * 1024 * 1024 >= min_zncc_q10 * min_zncc_q10 * var_ref * var_cur:
        return 0
    return 1


def take(levels, xyl):
    """patch (n,64) u8 and validity (n,) bool; levels = list of 2-D u8 arrays (one frame's pyramid, blurred or not)"""
    xyl = np.asarray(xyl, np.int64).reshape(-1, 3); n = len(xyl)
    patch = np.zeros((n, 64), np.uint8); valid = np.zeros(n, bool)
    for k, (x, y, l) in enumerate(xyl):
        if not 0 <= l < len(levels):
            continue
        h, w = levels[l].shape
        if x < 4 or x + 3 >= w or y < 4 or y + 3 >= h:
            continue
        patch[k] = levels[l][y - 4:y + 4, x - 4:x + 4].reshape(64); valid[k] = True
    return patch, valid


def patch_points(levels, xyl, ref_patch=None, min_var=0, min_zncc_q10=0):
    """(patch (n,64) u8, sums (n,3) i32 or None, status (n,) i32 or None): the three outputs of vido_orb_patch_points"""
    patch, valid = take(levels, xyl); n = len(patch)
    if ref_patch is None:
        return patch, None, None
    ref = np.asarray(ref_patch, np.uint8).reshape(n, 64)
    sm = np.zeros((n, 3), np.int32); st = np.full(n, -1, np.int32)
    for k in range(n):
        if not valid[k]:
            continue
        c, vr, vc = sums(ref[k], patch[k])
        assert abs(c) <= VAR_MAX and 0 <= vr <= VAR_MAX and 0 <= vc <= VAR_MAX
        sm[k] = (c, vr, vc); st[k] = verdict(c, vr, vc, min_var, min_zncc_q10)
    return patch, sm, st


def constructed():
    """name -> (reference patch, current patch) u8 (64,): the cases whose result follows from the definition alone"""
    rng = np.random.RandomState(7)
    rnd = rng.randint(0, 256, 64).astype(np.uint8)
    yy, xx = np.mgrid[0:8, 0:8]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8).reshape(64)
    ramp = (np.arange(64) * 4).astype(np.uint8)
    return {"identical": (rnd, rnd.copy()), "inverse": (rnd, (255 - rnd).astype(np.uint8)), "white": (np.full(64, 255, np.uint8), np.full(64, 255, np.uint8)),
            "checker": (checker, checker.copy()), "checker_inverse": (checker, (255 - checker).astype(np.uint8)), "ramp_vs_random": (ramp, rnd),
            "gain_offset": ((rnd // 2).astype(np.uint8), (rnd // 2 + 100).astype(np.uint8)), "flat_vs_random": (np.full(64, 17, np.uint8), rnd)}
