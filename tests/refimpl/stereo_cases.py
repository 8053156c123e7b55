"""Inputs for the tests of vido_stereo_sgm: a random texture with a random warp of it as the right view, and hostile pairs, each with the property of the statement's
output that shows the case is what its name says (so that a drifting generator cannot make a case vacuous)."""
import numpy as np

from . import stereo_sgm_np as G


def warped_pair(w, h, D, seed):
    """A random texture and a random warp of it: the right image at column x shows the texture's column x + d(y, x), d constant over 8 x 6 cells and spread over [0, D)"""
    rng = np.random.RandomState(seed)
    tex = rng.randint(0, 256, (h, w + D)).astype(np.uint8)
    d = np.repeat(np.repeat(rng.randint(0, D, ((h + 5) // 6, (w + 7) // 8)), 6, 0), 8, 1)[:h, :w]
    right = tex[np.arange(h)[:, None], np.arange(w)[None, :] + d]
    return np.ascontiguousarray(tex[:, :w]), np.ascontiguousarray(right)


def hostile_cases(w, h, D, seed=8):
    """[(name, left, right, params, shows(want, S, C) -> bool)]: want = the statement's (disp, q4, status, stats), S its summed volume, C its cost volume"""
    rng = np.random.RandomState(seed)
    n = w * h
    tex = rng.randint(0, 256, (h, w)).astype(np.uint8); noise = rng.randint(0, 256, (h, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    ties = lambda V: ((V == V.min(2, keepdims=True)).sum(2) > 1).mean()                              # share of pixels whose minimum over d is taken more than once
    # no texture: every cost inside the image is 0 and ties, and only the paths' memory of the left border (C = 64 where x - d < 0) prefers d = 0: zero disparity everywhere
    flat = lambda want, S, C: not want[1].any() and want[3][3] == n and ties(C) > 0.8
    rolled = lambda k: np.ascontiguousarray(np.roll(tex, -k, axis=1))                                 # the right view shows the left's column x + k: disparity k
    return [
        ("constant", np.full((h, w), 93, np.uint8), np.full((h, w), 93, np.uint8), {}, flat),
        ("all 0", np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), {}, flat),
        ("all 255", np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8), {}, flat),
        ("constant against noise", np.full((h, w), 93, np.uint8), noise, {}, lambda want, S, C: want[3][0] < 0.2 * n),
        ("period-2 checkerboard", checker, checker, {}, lambda want, S, C: ties(C) > 0.9 and not want[1].any()),                  # the costs tie at every other d
        ("period-2 checkerboard, no penalties", checker, checker, dict(p1=0, p2=0), lambda want, S, C: ties(S) > 0.9 and not want[1].any()),      # S = 8 C: the lowest d wins every tie
        ("unrelated noise", tex, noise, {}, lambda want, S, C: want[3][2] > 0.3 * n and want[3][0] < 0.5 * n),
        ("identical images", tex, tex, {}, lambda want, S, C: want[3][3] > 0.5 * n and (want[1] <= 0).mean() > 0.5),
        ("rolled by 5", tex, rolled(5), {}, lambda want, S, C: ((want[1] + 8) >> 4 == 5).mean() > 0.7 and want[3][0] > 0.7 * n),
        ("rolled by D - 1", tex, rolled(D - 1), {}, lambda want, S, C: (want[1] == 16 * (D - 1)).mean() > 0.3),
        ("rolled by D", tex, rolled(D), {}, lambda want, S, C: want[3][0] < 0.5 * n),
    ]


def run(left, right, **kw):
    """the statement's outputs, its S and its C"""
    p = {**G.DEFAULTS, **kw}
    C, _, S = G.volumes(left, right, p["max_disp"], p["p1"], p["p2"], p.get("rgb_order", 0))
    return G.select(S, p["uniqueness"], p["lr_tol"]), S, C
