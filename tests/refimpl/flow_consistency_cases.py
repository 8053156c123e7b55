"""Constructed inputs of vido_flow_consistency shared by tests/test_flow_consistency_cpu.py (the statement against Python integers) and tests/test_flow_consistency_gpu.py
(the kernel against the statement), and an independent per-pixel form of the rule in Python integers.  Each case: (name, fwd i32 [H][W][2], bwd, alpha_q10, beta_q16)."""
import numpy as np

TOP = (1 << 19) - 1                                # the largest component that still is a flow


def pixel(fwd, bwd, x, y, alpha_q10, beta_q16, terms=None):
    """(status, b or None) of one pixel in Python integers, written from the definition alone; terms: a list that collects every intermediate's magnitude"""
    h, w = fwd.shape[:2]
    note = (lambda *v: terms.extend(abs(int(t)) for t in v)) if terms is not None else (lambda *v: None)
    fx, fy = int(fwd[y, x, 0]), int(fwd[y, x, 1])
    if abs(fx) >= 1 << 19 or abs(fy) >= 1 << 19:
        return 3, None
    tx, ty = 256 * x + fx, 256 * y + fy
    if tx < 0 or tx > 256 * (w - 1) or ty < 0 or ty > 256 * (h - 1):
        return 2, None
    x0, ax, y0, ay = tx >> 8, tx & 255, ty >> 8, ty & 255
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    taps = [[int(v) for v in bwd[j, i]] for j, i in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
    if any(abs(v) >= 1 << 19 for t in taps for v in t):
        return 3, None
    wts = ((256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay)
    s = [sum(wt * t[c] for wt, t in zip(wts, taps)) for c in (0, 1)]
    b = [(v + 32768) >> 16 for v in s]                                   # Python's >> floors, like an arithmetic shift
    r = (fx + b[0], fy + b[1])
    lhs = 1024 * (r[0] * r[0] + r[1] * r[1])
    rhs = alpha_q10 * (fx * fx + fy * fy + b[0] * b[0] + b[1] * b[1]) + 1024 * beta_q16
    note(*s, *b, *r, lhs, rhs, alpha_q10 * (fx * fx + fy * fy + b[0] * b[0] + b[1] * b[1]), 1024 * beta_q16)
    return (1 if lhs > rhs else 0), b


def by_pixels(fwd, bwd, alpha_q10, beta_q16, terms=None):
    """The status image through pixel()"""
    h, w = fwd.shape[:2]
    return np.array([[pixel(fwd, bwd, x, y, alpha_q10, beta_q16, terms)[0] for x in range(w)] for y in range(h)], np.uint8)


def _z(h, w):
    return np.zeros((h, w, 2), np.int32)


def borders(h, w):
    """Targets exactly on the last column / row (in), one past them (out) and at -1 (out); the backward field is 0, alpha = 1: 1024 |f|^2 <= 1024 |f|^2 keeps every target
    that is in.  Returns the case and the expected status image."""
    f, want = _z(h, w), np.zeros((h, w), np.uint8)
    f[0, w - 2, 0] = 256; f[1, w - 2, 0] = 257; want[1, w - 2] = 2       # tx = 256 (w - 1), and one past it
    f[2, 0, 0] = -1; want[2, 0] = 2                                       # tx = -1
    f[h - 2, 1, 1] = 256; f[h - 2, 2, 1] = 257; want[h - 2, 2] = 2        # ty = 256 (h - 1), and one past it
    f[0, 2, 1] = -1; want[0, 2] = 2                                       # ty = -1
    f[h - 1, w - 1] = (0, 0)                                              # the corner itself: x1 and y1 both clamp
    return ("borders %dx%d" % (w, h), f, _z(h, w), 1024, 0), want


def clamps_and_fractions(h, w, seed):
    """A random backward field under targets on the last column and row (x1 / y1 clamped), at ax = ay = 255 and at random fractions"""
    rng = np.random.RandomState(seed)
    b = rng.randint(-700, 701, (h, w, 2)).astype(np.int32)
    f = rng.randint(-300, 301, (h, w, 2)).astype(np.int32)
    f[1, 1] = (255, 255)                                                  # ax = ay = 255
    f[2, 1] = (-1, -1)                                                    # ax = ay = 255 from the other side
    f[1, w - 2] = (256, 0); f[h - 2, 1] = (0, 256); f[h - 2, w - 2] = (256, 256); f[h - 1, w - 1] = (0, 0); f[h - 1, w - 2] = (200, 0); f[h - 2, w - 1] = (0, 200)
    return ("clamps %dx%d" % (w, h), f, b, 10, 32768)


def negative_rounding(h, w):
    """s = 32768 (B00 + B01) at ax = 128, ay = 0: the sums -1, -3, 3, 1, -2 give b = 0, -1, 2, 1, -1 — (s + 32768) >> 16 rounds halves up, also below zero.  Returns the
    case, the pixels and the b.x each must get."""
    f, b = _z(h, w), _z(h, w)
    sums, want = (-1, -3, 3, 1, -2), (0, -1, 2, 1, -1)
    for k, s in enumerate(sums):                                          # pixel (0, k): target x = 0.5 between columns 0 and 1 of row k
        f[k % h, 0] = (128, 0)
    rows = min(h, len(sums))
    for k in range(rows):
        b[k, 0, 0] = sums[k] - 7; b[k, 1, 0] = 7
    return ("negative rounding %dx%d" % (w, h), f, b, 0, 1 << 30), [(0, k) for k in range(rows)], want[:rows]


def extremes(h, w):
    """Taps of +-(2^19 - 1) under in-image targets, forward components of +-(2^19 - 1) (which leave a small image), at the largest alpha and beta; and +-2^19 in the
    forward field and in a single tap"""
    f, b = _z(h, w), _z(h, w)
    b[0, 0] = (TOP, TOP); b[0, 1] = (TOP, -TOP); b[1, 0] = (-TOP, TOP); b[1, 1] = (-TOP, -TOP)
    f[0, 0] = (128, 128); f[0, 1] = (0, 0); f[1, 0] = (10, 0); f[1, 1] = (0, 255)
    f[2, 2] = (TOP, 0); f[1, 3] = (0, -TOP); f[1, 2] = (-TOP, TOP)
    f[3, 0] = (1 << 19, 0); f[3, 1] = (0, -(1 << 19)); f[3, 2] = (-(1 << 19), 1 << 19); f[2, 0] = (np.iinfo(np.int32).min, 0); f[2, 1] = (0, np.iinfo(np.int32).max)
    b[h - 1, w - 1] = (0, 1 << 19)                                        # a single tap: the pixels that target it, through any of their four taps
    f[h - 1, w - 2] = (256, 0); f[h - 2, w - 1] = (0, 128)
    return ("extremes %dx%d" % (w, h), f, b, 1024, 1 << 30)


def widest():
    """1 x 4095: the only kind of field in which a forward component of +-(2^19 - 1) stays inside, against taps of the same size and sign (the largest |r|), and of the
    opposite sign (r = 0)"""
    w = 4095
    f, b = _z(1, w), _z(1, w)
    same, opposite = (0, w - 81), (40, w - 121)                          # (far enough apart that no two of them share a tap)
    for x in same + opposite:
        f[0, x, 0] = TOP if x < w // 2 else -TOP
        t = (256 * x + int(f[0, x, 0])) >> 8
        b[0, t:t + 2, 0] = f[0, x, 0] if x in same else -f[0, x, 0]
        b[0, t:t + 2, 1] = TOP if x in same else 0
    return ("widest 4095x1", f, b, 1024, 1 << 30)


def exact_only(h, w):
    """alpha = beta = 0 passes only r = 0: a 1-px translation and its negation, with one backward vector off by 1/256 px"""
    f, b = _z(h, w), _z(h, w)
    f[..., 0] = 256; b[..., 0] = -256
    b[1, 2, 0] = -255                                                     # pixel (1, 1) targets (2, 1): r = (1, 0)
    return ("exact only %dx%d" % (w, h), f, b, 0, 0)


def translation(h, w, dx, dy):
    """A forward field that is an exact integer translation and its negation"""
    f, b = _z(h, w), _z(h, w)
    f[..., 0] = 256 * dx; f[..., 1] = 256 * dy; b[..., 0] = -256 * dx; b[..., 1] = -256 * dy
    return f, b


def random_fields(h, w, seed):
    """Magnitudes up to 2^19 - 1 on a log scale (so that many targets stay inside), a sprinkling at +-2^19"""
    rng = np.random.RandomState(seed)
    def field():
        mag = np.exp2(rng.uniform(0, 19, (h, w, 2))).astype(np.int64).clip(0, TOP)
        v = (mag * rng.choice((-1, 1), (h, w, 2))).astype(np.int32)
        hit = rng.rand(h, w, 2) < 0.01
        v[hit] = rng.choice((-(1 << 19), 1 << 19), int(hit.sum()))
        top = rng.rand(h, w, 2) < 0.01
        v[top] = rng.choice((-TOP, TOP), int(top.sum()))
        return v
    return field(), field()


def constructed():
    """Every constructed case at 5 x 4 and 16 x 16, and the 4095 x 1 one"""
    out = []
    for h, w in ((4, 5), (16, 16)):
        out += [borders(h, w)[0], clamps_and_fractions(h, w, 3 + w), negative_rounding(h, w)[0], extremes(h, w), exact_only(h, w)]
    return out + [widest()]
