"""Overlap association of a warped label image with a detector's instance image, stated in plain numpy: the reference of vido_mask_associate (include/vido_c.h).

associate(prev, cur, n, classes, hold, state) -> (out int32 [H,W], lut int32 [256], state int32 [768] (a new array), stats int32 [4] = matched, fresh, lost, left out)

  prev     int32 [H,W] or None (all zero): the previous handed-over label image warped into this frame (ids 1..254)
  cur      int32 [H,W]: the detector's instance image at id base 0, value 1 + slot
  n        number of slots, <= 127;  classes int64 [n] or None (every slot live);  hold >= 0
  state    int32 [768]: [0] the cursor, [256 + id] the class of id (nonzero exactly when the id is live or held), [512 + id] the frames the id has been lost; zeros = new sequence

  0. p = prev where 1 <= prev <= 254 else 0;  c = cur where 1 <= cur <= n and classes[cur - 1] != 0 else 0
  1. C[p][c] = pixels with that pair;  Ap[p] = sum_c C[p][c] (p >= 1),  Ac[c] = sum_p C[p][c] (c >= 1), zero column / row included
  2. c with Ac[c] > 0 matches the p >= 1 with 2 C[p][c] > Ap[p] + Ac[c] - C[p][c]  (IoU > 1/2)
  3. every unmatched c with Ac[c] > 0, ascending: the next id after the cursor, cyclic over 1..254, with Ap[id] == 0 and not handed out in this call; cursor = id.
     None free: the instance gets 0 (left out), the cursor stays.  A cursor outside 0..254 reads as 0.
  4. LUT[c] = the matched p, the fresh id or 0;  an assigned id takes class[id] = classes[c - 1] (1 without classes; the low 32 bits), lost[id] = 0
  5. p with Ap[p] > 0 that nothing matched: lost[p] += 1; lost[p] <= hold: KEEP[p] = p (held), else KEEP[p] = 0 and class[p] = lost[p] = 0.
     Ids with Ap == 0 that were not assigned in this call: class = lost = 0.
  6. out = LUT[c] where nonzero, else KEEP[p]

Why step 2 needs no order and no tie rule.  Write I = C[p][c].  A match means 3 I > Ap[p] + Ac[c].
  one p per c:  Ap[p] >= I, so 3 I > I + Ac[c], i.e. I > Ac[c] / 2: p holds more than half of c's pixels.  Two different p cannot both hold more than half of them
                (their pixel sets within c are disjoint), so at most one p matches c — and it is the strict maximum of column c over p >= 1.
  one c per p:  Ac[c] >= I, so in the same way I > Ap[p] / 2: c holds more than half of p's pixels, and two different c cannot.
So the matched pairs form a partial one-to-one map whatever order the pairs are looked at.  All counts are at most 4095 * 4095 < 2^24, so 3 I fits 32 unsigned bits.
"""
import numpy as np

N_IDS = 254
MAX_SLOTS = 127
STATE_WORDS = 768


def clean(prev, cur, n, classes):
    """Step 0 -> (p, c) as int64 images."""
    cur = np.asarray(cur)
    assert cur.dtype == np.int32 and cur.ndim == 2 and 0 <= n <= MAX_SLOTS
    if prev is None:
        p = np.zeros(cur.shape, np.int64)
    else:
        prev = np.asarray(prev)
        assert prev.dtype == np.int32 and prev.shape == cur.shape
        p = np.where((prev >= 1) & (prev <= N_IDS), prev, 0).astype(np.int64)
    live = np.zeros(256, bool)
    for s in range(n):
        live[1 + s] = True if classes is None else int(classes[s]) != 0
    c64 = cur.astype(np.int64)
    ok = (c64 >= 1) & (c64 <= n)
    c = np.where(ok & live[np.where(ok, c64, 0)], c64, 0)
    return p, c


def associate(prev, cur, n, classes, hold, state):
    assert hold >= 0
    state = np.asarray(state)
    assert state.dtype == np.int32 and state.shape == (STATE_WORDS,)
    if classes is not None:
        classes = np.asarray(classes)
        assert classes.dtype == np.int64 and classes.shape[0] >= n
    p, c = clean(prev, cur, n, classes)
    # 1. the count table and its sums
    C = np.bincount((p * 256 + c).ravel(), minlength=65536).reshape(256, 256).astype(np.int64)
    Ap = C.sum(1); Ac = C.sum(0)
    Ap[0] = 0; Ac[0] = 0
    # 2. matches
    lut = np.zeros(256, np.int64)
    matched_p = np.zeros(256, bool)
    for ci in range(1, n + 1):
        if Ac[ci] == 0:
            continue
        hits = [pi for pi in range(1, N_IDS + 1) if 3 * C[pi, ci] > Ap[pi] + Ac[ci]]
        assert len(hits) <= 1                                            # (the docstring's argument)
        if hits:
            assert not matched_p[hits[0]]
            lut[ci] = hits[0]; matched_p[hits[0]] = True
    n_matched = int(matched_p.sum())
    # 3. fresh ids
    cursor = int(state[0])
    if not 0 <= cursor <= N_IDS:
        cursor = 0
    handed = np.zeros(256, bool)
    n_fresh = n_left = 0
    for ci in range(1, n + 1):
        if Ac[ci] == 0 or lut[ci] != 0:
            continue
        for j in range(1, N_IDS + 1):
            cand = (cursor - 1 + j) % N_IDS + 1 if cursor >= 1 else j    # the ids after the cursor, in cyclic order (cursor 0: 1, 2, ...)
            if Ap[cand] == 0 and not handed[cand]:
                lut[ci] = cand; handed[cand] = True; cursor = cand; n_fresh += 1
                break
        else:
            n_left += 1
    # 4. + 5. the state
    cls = state[256:512].astype(np.int64).copy(); lost = state[512:768].astype(np.int64).copy()
    assigned = np.zeros(256, bool)
    for ci in range(1, n + 1):
        if lut[ci]:
            i = int(lut[ci])
            assigned[i] = True
            cls[i] = 1 if classes is None else int(np.int64(classes[ci - 1]).astype(np.int32))
            lost[i] = 0
    keep = np.zeros(256, np.int64)
    n_lost = 0
    for pi in range(1, N_IDS + 1):
        if assigned[pi]:
            continue
        if Ap[pi] > 0:
            n_lost += 1
            lost[pi] += 1
            if lost[pi] <= hold:
                keep[pi] = pi
                continue
        cls[pi] = 0; lost[pi] = 0
    new_state = state.copy()
    new_state[0] = cursor
    new_state[256:512] = cls.astype(np.int32); new_state[512:768] = lost.astype(np.int32)
    # 6. the image
    out = lut[c]
    out = np.where(out != 0, out, keep[p]).astype(np.int32)
    return out, lut.astype(np.int32), new_state, np.array([n_matched, n_fresh, n_lost, n_left], np.int32)
