"""Class label images for the connected-component tests (tests/test_mask_components_cpu.py, tests/test_mask_components_gpu.py): each is a place where component
labelling breaks — a tile seam, a long chain, a corner, a flood of components.  Every generator takes (H, W) and works at any size, 1 x N and N x 1 included."""
import numpy as np

TILE = 32                                                            # the product's tile edge (csrc/maskcc.hip): the seams the patterns aim at


def blobs(H, W, seed, hostile=True):
    """Rectangles and discs of a few values painted over each other (equal values that touch join, different ones never do), then sprinkled with values that read as
    background (<= 0) and with huge positive classes that are components of their own."""
    rng = np.random.RandomState(seed)
    m = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    values = (3, 3, 7, 1, 2147483647, 3, 41, 7)
    for i in range(14):
        cy, cx = rng.randint(0, H), rng.randint(0, W); ry, rx = rng.randint(2, max(3, H // 4)), rng.randint(2, max(3, W // 5))
        where = (np.abs(yy - cy) < ry) & (np.abs(xx - cx) < rx) if i & 1 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        m[where] = values[i % len(values)]
    if hostile:
        for v in (0, -1, -2147483648, 2147483647, 2147483646, 255, 65536):
            m[rng.rand(H, W) < 0.006] = v
    return m


def full(H, W):
    return np.full((H, W), 9, np.int32)


def empty(H, W):
    return np.zeros((H, W), np.int32)


def checkerboard(H, W):
    """8-connected: one component; 4-connected: every foreground pixel its own."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, 5, 0).astype(np.int32)


def _spiral(n, off, pitch, value, m):
    """A one-pixel line from (off, off) inwards: right, down, left, up, ... with segment lengths L, L, L, L - p, L - p, L - 2p, L - 2p, ..."""
    L = n - 1 - 2 * off
    x = y = off
    if L < 0:
        return
    m[y, x] = value
    lengths = [L, L, L]
    k = 1
    while L - k * pitch > 0:
        lengths += [L - k * pitch] * 2
        k += 1
    for s, ln in enumerate(lengths):
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[s % 4]
        for _ in range(ln):
            x += dx; y += dy
            m[y, x] = value


def spirals(H, W):
    """Two interleaved one-pixel spirals of different values, pitch 4, the second shifted by (2, 2): two components whose chains wind through every tile."""
    n = min(H, W)
    m = np.zeros((H, W), np.int32)
    if n >= 8:
        _spiral(n, 0, 4, 11, m)
        _spiral(n, 2, 4, 12, m)
    else:
        m[0, :] = 11
    return m


def serpentine(H, W):
    """One line, one pixel wide: every even row in full, joined at alternating ends — it crosses every vertical seam in every even row and every horizontal seam."""
    m = np.zeros((H, W), np.int32)
    m[0::2, :] = 6
    for y in range(1, H - 1, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 6
    return m


def comb(H, W):
    """Teeth on every other column that join only in the last row: the anchors merge at the very end."""
    m = np.zeros((H, W), np.int32)
    m[:, 0::2] = 8
    m[H - 1, :] = 8
    return m


def corner_touch(H, W, anti=False):
    """Two equal-valued squares that touch at a tile corner only: (31, 31) and (32, 32), or with anti (31, 32) and (32, 31).  8-connected: one; 4-connected: two."""
    m = np.zeros((H, W), np.int32)
    t = TILE
    if anti:
        m[max(t - 9, 0):t, t:t + 9] = 4
        m[t:t + 9, max(t - 9, 0):t] = 4
    else:
        m[max(t - 9, 0):t, max(t - 9, 0):t] = 4
        m[t:t + 9, t:t + 9] = 4
    return m
