"""The windowed descriptor matcher stated in plain numpy: the reference of vido_hamming_match_window (include/vido_c.h).

match_window(q_desc, q_xy, q_level, t_desc, t_xy, t_level, radius, level_tol=1, max_dist=256, ratio=None, unique=False)
    -> (idx int32 [nq], dist int32 [nq], dist2 int32 [nq], status int32 [nq], stats int32 [5])

  q_desc / t_desc  uint8 [n,32];  q_xy / t_xy  float32 [n,2];  q_level / t_level  int32 [n]
  ratio            None (off) or (num, den) with 0 < num <= den <= 1024 (ValueError otherwise, as for a radius that is negative, NaN or infinite)

A double loop over queries and train entries (the tests of one query's row are written as array expressions, its candidates are walked one by one in ascending j), then
one pass for the one-to-one rule:
  candidate   |tx - qx| <= radius and |ty - qy| <= radius, every term ONE float32 subtraction and one compare (NaN and inf coordinates fail), and
              level_tol < 0 or |t_level - q_level| <= level_tol
  best        smallest Hamming distance, the FIRST j that reaches it;  dist2: the smallest distance among the other candidates;  -1 where there is none
  status      1 no candidate | 2 dist > max_dist | 3 ratio on, dist2 >= 0 and not dist * den < dist2 * num | 4 unique and the claim lost | 0 matched — the first that fires
  unique      among the queries that arrive at this test with the same best j the smallest (dist, i) keeps it, all others get 4
  idx         j for status 0, else -1;  stats[s] = number of queries with status s
"""
import numpy as np

_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def match_window(q_desc, q_xy, q_level, t_desc, t_xy, t_level, radius, level_tol=1, max_dist=256, ratio=None, unique=False):
    q_desc = np.asarray(q_desc, np.uint8).reshape(-1, 32); t_desc = np.asarray(t_desc, np.uint8).reshape(-1, 32)
    q_xy = np.asarray(q_xy, np.float32).reshape(-1, 2); t_xy = np.asarray(t_xy, np.float32).reshape(-1, 2)
    q_level = np.asarray(q_level, np.int32).reshape(-1); t_level = np.asarray(t_level, np.int32).reshape(-1)
    nq, nt = len(q_desc), len(t_desc)
    assert len(q_xy) == nq and len(q_level) == nq and len(t_xy) == nt and len(t_level) == nt
    radius = np.float32(radius)
    if not (radius >= 0 and np.isfinite(radius)):
        raise ValueError("radius")
    num, den = (0, 1) if ratio is None else (int(ratio[0]), int(ratio[1]))
    if ratio is not None and not (0 < num <= den <= 1024):
        raise ValueError("ratio")
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, -1, np.int32); dist2 = np.full(nq, -1, np.int32); status = np.zeros(nq, np.int32)
    best_j = np.full(nq, -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nq):
            d1, d2, j1 = -1, -1, -1
            # the two tests of every (i, j), row i at once: float32 arrays subtract element by element in float32, levels in int64
            ok = (np.abs(t_xy[:, 0] - q_xy[i, 0]) <= radius) & (np.abs(t_xy[:, 1] - q_xy[i, 1]) <= radius)
            if level_tol >= 0:
                ok &= np.abs(t_level.astype(np.int64) - int(q_level[i])) <= level_tol
            for j in np.flatnonzero(ok):                                # ascending j
                d = hamming(q_desc[i], t_desc[j])
                if d1 < 0 or d < d1:
                    d2, d1, j1 = d1, d, j
                elif d2 < 0 or d < d2:
                    d2 = d
            dist[i], dist2[i], best_j[i] = d1, d2, j1
            if d1 < 0:
                status[i] = 1
            elif d1 > max_dist:
                status[i] = 2
            elif num > 0 and d2 >= 0 and not (d1 * den < d2 * num):
                status[i] = 3
    if unique:
        owner = {}
        for i in range(nq):
            if status[i] == 0:
                k = (int(dist[i]), i)
                if best_j[i] not in owner or k < owner[best_j[i]]:
                    owner[best_j[i]] = k
        for i in range(nq):
            if status[i] == 0 and owner[best_j[i]] != (int(dist[i]), i):
                status[i] = 4
    idx[status == 0] = best_j[status == 0]
    stats = np.bincount(status, minlength=5).astype(np.int32)
    return idx, dist, dist2, status, stats
