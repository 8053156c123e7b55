"""MI355X: vido_mask_associate (csrc/maskassoc.hip) against the numpy statement of the rule (tests/refimpl/mask_associate_np.py): bit-exact label image, lookup table,
state and counters on seeded blob images with hostile values, three sizes, four instance counts, no previous image, one label everywhere, a chained sequence across the
cursor's wrap, in-place output, unaligned buffers, graph replay and the refusals.  Every reference is computed once (REF) and never modified."""
import ctypes as C

import numpy as np
import pytest
import torch

from refimpl.mask_associate_np import associate, STATE_WORDS

pytestmark = pytest.mark.gpu

CTX_W, CTX_H = 1242, 375
SIZES = ((64, 64), (201, 151), (375, 1242))    # H, W
COUNTS = (0, 1, 5, 127)
REF = {}


def blob_pair(H, W, n, seed, hostile=True):
    """n blobs (rectangles and discs).  prev paints blob i under a distinct id of 1..254 (a fifth of the blobs are new: not in prev; a few ids of prev have no blob in cur);
    cur paints it shifted by 0-6 px under slot value 1 + perm[i].  hostile: both images sprinkled with values that must read as background, and some classes are 0."""
    rng = np.random.RandomState(seed)
    prev = np.zeros((H, W), np.int32); cur = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    ids = rng.permutation(254)[:n + 3] + 1
    perm = rng.permutation(n)
    for i in range(n + 3):
        cy, cx = rng.randint(0, H), rng.randint(0, W); ry, rx = rng.randint(3, max(4, H // 5)), rng.randint(3, max(4, W // 6))
        dy, dx = rng.randint(0, 7, 2) * rng.choice((-1, 1), 2)
        shape = (lambda oy, ox: (np.abs(yy - cy - oy) < ry) & (np.abs(xx - cx - ox) < rx)) if i & 1 else (lambda oy, ox: ((yy - cy - oy) / ry) ** 2 + ((xx - cx - ox) / rx) ** 2 < 1)
        if i >= n or rng.rand() > 0.2:
            prev[shape(0, 0)] = ids[i]
        if i < n:
            cur[shape(dy, dx)] = 1 + perm[i]
    classes = rng.randint(1, 80, n).astype(np.int64)
    if hostile:
        for v in (255, -3, 300, -2147483648, 256):
            prev[rng.rand(H, W) < 0.004] = v
        for v in (n + 1, -4, 2147483647, 128, 255, 256):
            cur[rng.rand(H, W) < 0.004] = v
        classes[rng.rand(n) < 0.1] = 0
    state = np.zeros(STATE_WORDS, np.int32)
    state[0] = rng.randint(0, 255)
    for i in ids:                                                     # the ids of prev are known to the state; some have been lost for a frame already
        state[256 + i] = rng.randint(1, 80); state[512 + i] = rng.randint(0, 2)
    return prev, cur, classes, state


def reference(key, make, hold):
    if key not in REF:
        prev, cur, classes, state = make()
        for a in (prev, cur, classes, state):
            if a is not None:
                a.setflags(write=False)
        n = len(classes) if classes is not None else 127
        REF[key] = (prev, cur, classes, state, associate(prev, cur, n, classes, hold, state))
    return REF[key]


@pytest.fixture(scope="module")
def ops(vido):
    from vido_slam_amd import nets
    ctx = vido.Context(width=CTX_W, height=CTX_H, max_batch=1)
    yield nets.HipOps(ctx)
    torch.cuda.synchronize()
    ctx.close()


def dev(a, offset=0):
    """A device copy of `a` that starts `offset` elements behind an allocation's start (offset 1: 4-byte aligned only)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    if offset:
        buf = torch.empty((t.numel() + offset,), dtype=t.dtype, device="cuda")
        v = buf[offset:].view(t.shape); v.copy_(t)
        return v
    return t


def run(ops, prev, cur, classes, hold, state, n=None, alias=False, offsets=(0, 0, 0)):
    """-> (out, lut, state, stats) as numpy, with out / lut / stats pre-filled with garbage; the inputs are checked to be untouched"""
    tp, tc, tk, ts = dev(prev, offsets[0]), dev(cur, offsets[1]), dev(classes), dev(state)
    out = tc if alias else dev(np.full(cur.shape, -559038737, np.int32), offsets[2])
    lut = torch.full((256,), 12345, dtype=torch.int32, device="cuda"); st = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
    r = ops.mask_associate(tp, tc, ts, classes=tk, n=n, hold=hold, out=out, lut=lut, stats=st)
    assert r is out
    torch.cuda.synchronize()
    if prev is not None:
        assert np.array_equal(tp.cpu().numpy(), prev)
    if not alias:
        assert np.array_equal(tc.cpu().numpy(), cur)
    return out.cpu().numpy(), lut.cpu().numpy(), ts.cpu().numpy(), st.cpu().numpy()


def same(got, ref, what=""):
    for name, g, r in zip(("out", "lut", "state", "stats"), got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r), "%s %s: %d elements differ" % (what, name, int((g != r).sum()))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("H,W", SIZES)
def test_bit_exact_on_hostile_blob_images(ops, H, W, n):
    """Two different inputs back to back through one context: a count left in the table by the call before would show in the next result."""
    tot = np.zeros(4, np.int64)
    for seed in (21, 22):
        prev, cur, classes, state, ref = reference((H, W, n, seed), lambda: blob_pair(H, W, n, seed + 1000 * H + n), hold=1)
        got = run(ops, prev, cur, classes, 1, state)
        print("%dx%d n=%d seed %d: stats %s, reference %s, cursor %d -> %d" % (H, W, n, seed, got[3].tolist(), ref[3].tolist(), state[0], ref[2][0]))
        same(got, ref, "seed %d" % seed)
        tot += ref[3]
    if n >= 5:
        assert tot[0] > 0 and tot[1] > 0                              # the cases hold matches and fresh ids
    assert tot[2] > 0                                                 # and ids of prev that nothing matched


def test_without_a_previous_image_and_without_classes(ops):
    H, W = 201, 151
    def make():
        _, cur, _, state = blob_pair(H, W, 5, 77, hostile=False)
        return None, cur, None, state
    _, cur, _, state, ref = reference(("noprev",), make, hold=3)
    assert state[256:].any()
    got = run(ops, None, cur, None, 3, state, n=127)
    same(got, ref)
    assert ref[3][0] == 0 and ref[3][1] >= 1 and ref[3][2] == 0       # fresh ids only; the ids the state knew are gone from the image and cleared, whatever the hold
    assert int((ref[2][256:512] != 0).sum()) == ref[3][1]


def test_one_label_everywhere(ops):
    """Every pixel is the pair (9, 1): every add of every wave lands on one counter.  IoU 1: the instance takes over id 9."""
    H, W = 375, 1242
    prev = np.full((H, W), 9, np.int32); cur = np.ones((H, W), np.int32)
    state = np.zeros(STATE_WORDS, np.int32); state[0] = 9; state[256 + 9] = 3
    ref = associate(prev, cur, 1, np.array([4], np.int64), 0, state)
    got = run(ops, prev, cur, np.array([4], np.int64), 0, state)
    same(got, ref)
    assert (got[0] == 9).all() and got[3].tolist() == [1, 0, 0, 0] and got[2][256 + 9] == 4
    # all background: nothing is added anywhere
    z = np.zeros((H, W), np.int32)
    got = run(ops, z, z, np.array([4], np.int64), 2, state)
    same(got, associate(z, z, 1, np.array([4], np.int64), 2, state))
    assert not got[0].any() and got[3].tolist() == [0, 0, 0, 0]


def test_six_frames_chained_through_one_state_across_the_wrap(ops):
    """Blobs that move 3 px a frame; the detector permutes its slots every frame, misses blob 0 on frames 2 and 3 (hold = 2 keeps it) and sees a new blob from frame 4 on.
    The device's state and image are fed back frame after frame and never corrected from the reference; cursor 252 at the start, so the fresh ids cross 254 -> 1."""
    H, W, nb = 151, 201, 5
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W]
    cen = [(30 + 22 * i, 25 + 30 * i) for i in range(nb + 1)]
    state_ref = np.zeros(STATE_WORDS, np.int32); state_ref[0] = 252
    state_dev = torch.from_numpy(state_ref.copy()).cuda()
    prev_ref = None; prev_dev = None
    ids_of = []
    for k in range(6):
        present = [i for i in range(nb + 1) if (i < nb or k >= 4) and not (i == 0 and k in (2, 3))]
        perm = rng.permutation(len(present))
        cur = np.zeros((H, W), np.int32)
        for s, i in zip(perm, present):
            cur[(np.abs(yy - cen[i][0]) < 9) & (np.abs(xx - cen[i][1] - 3 * k) < 12)] = 1 + s
        classes = np.full(len(present), 3, np.int64)
        if prev_ref is not None:                                      # the "warp": frame k - 1's image moved by the 3 px the blobs move (the device's own image on its side)
            prev_ref = np.roll(prev_ref, 3, axis=1); prev_ref[:, :3] = 0
            prev_dev = torch.roll(out, 3, dims=1).contiguous(); prev_dev[:, :3] = 0
        out_ref, lut_ref, state_ref, stats_ref = associate(prev_ref, cur, len(present), classes, 2, state_ref)
        out = torch.empty((H, W), dtype=torch.int32, device="cuda"); stats = torch.zeros((4,), dtype=torch.int32, device="cuda")
        ops.mask_associate(prev_dev, torch.from_numpy(cur).cuda(), state_dev, classes=torch.from_numpy(classes).cuda(), hold=2, out=out, stats=stats)
        torch.cuda.synchronize()
        print("frame %d: stats %s, cursor %d, ids %s" % (k, stats.tolist(), int(state_dev[0]), sorted(set(np.unique(out_ref).tolist()) - {0})))
        assert np.array_equal(out.cpu().numpy(), out_ref) and np.array_equal(state_dev.cpu().numpy(), state_ref) and np.array_equal(stats.cpu().numpy(), stats_ref)
        ids_of.append({i: int(out_ref[cen[i][0], cen[i][1] + 3 * k]) for i in range(nb + 1)})
        prev_ref = out_ref
    assert sorted(ids_of[0][i] for i in range(nb)) == [1, 2, 3, 253, 254]           # handed out across the wrap
    for i in range(nb):
        assert len({f[i] for f in ids_of}) == 1, (i, [f[i] for f in ids_of])       # one id per blob over the six frames, blob 0 through its two missed frames
    assert ids_of[3][nb] == 0 and ids_of[4][nb] == ids_of[5][nb] == 4               # the newcomer takes the next id


def test_output_in_place_and_unaligned_buffers(ops):
    H, W = 201, 151                                                    # an odd width and an odd pixel count: scalar head and tail
    prev, cur, classes, state, ref = reference((H, W, 5, 21), lambda: blob_pair(H, W, 5, 21 + 1000 * H + 5), hold=1)
    same(run(ops, prev, cur, classes, 1, state, alias=True), ref, "out is cur")
    same(run(ops, prev, cur, classes, 1, state, offsets=(1, 1, 1)), ref, "4-byte aligned, all three alike")
    same(run(ops, prev, cur, classes, 1, state, offsets=(3, 3, 3)), ref, "12 bytes off a boundary")
    same(run(ops, prev, cur, classes, 1, state, offsets=(0, 1, 2)), ref, "three different alignments")
    same(run(ops, prev, cur, classes, 1, state, alias=True, offsets=(2, 2, 0)), ref, "in place, 8 bytes off")


def test_graph_replay_equals_eager(ops):
    H, W = 201, 151
    cases = [reference((H, W, 5, seed), lambda: blob_pair(H, W, 5, seed + 1000 * H + 5), hold=1) for seed in (21, 22)]
    sp = torch.zeros((H, W), dtype=torch.int32, device="cuda"); sc = torch.zeros((H, W), dtype=torch.int32, device="cuda"); sk = torch.ones((5,), dtype=torch.int64, device="cuda")
    sst = torch.zeros((STATE_WORDS,), dtype=torch.int32, device="cuda"); so = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    sl = torch.zeros((256,), dtype=torch.int32, device="cuda"); ss = torch.zeros((4,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.mask_associate(sp, sc, sst, classes=sk, hold=1, out=so, lut=sl, stats=ss)      # the warm-up call: the count table exists before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_associate(sp, sc, sst, classes=sk, hold=1, out=so, lut=sl, stats=ss)
    for prev, cur, classes, state, ref in cases:
        sp.copy_(torch.from_numpy(prev.copy())); sc.copy_(torch.from_numpy(cur.copy())); sk.copy_(torch.from_numpy(classes.copy())); sst.copy_(torch.from_numpy(state.copy()))
        so.fill_(-7); sl.fill_(-7); ss.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        same((so.cpu().numpy(), sl.cpu().numpy(), sst.cpu().numpy(), ss.cpu().numpy()), ref, "replay")


def test_refusals(ops):
    from vido_slam_amd.host import VidoError
    m = torch.zeros((64, 64), dtype=torch.int32, device="cuda"); c = torch.zeros((64, 64), dtype=torch.int32, device="cuda")
    s = torch.zeros((STATE_WORDS,), dtype=torch.int32, device="cuda"); k = torch.ones((5,), dtype=torch.int64, device="cuda")
    for bad in (lambda: ops.mask_associate(m, c, s, out=m),                                   # out aliases prev
                lambda: ops.mask_associate(m, c, s, out=torch.zeros((64, 63), dtype=torch.int32, device="cuda")),      # a wrong shape
                lambda: ops.mask_associate(None, c.view(-1)[:64 * 63].view(64, 63), s, out=c.view(-1)[4:4 + 64 * 63].view(64, 63)),      # out overlaps cur without being cur
                lambda: ops.mask_associate(m.cpu(), c, s), lambda: ops.mask_associate(m, c.cpu(), s), lambda: ops.mask_associate(m, c, s.cpu()),
                lambda: ops.mask_associate(m, c.to(torch.int64), s), lambda: ops.mask_associate(m, c, s.to(torch.int64)),
                lambda: ops.mask_associate(m, c, s, classes=k.to(torch.int32)), lambda: ops.mask_associate(m, c, s, classes=k, n=6),
                lambda: ops.mask_associate(m, c, s[:700]), lambda: ops.mask_associate(m[:, :63], c, s), lambda: ops.mask_associate(m, c.t(), s),
                lambda: ops.mask_associate(m, None, s), lambda: ops.mask_associate(m, c, None),
                lambda: ops.mask_associate(m, c, s, lut=torch.zeros((255,), dtype=torch.int32, device="cuda")),
                lambda: ops.mask_associate(m, c, s, stats=torch.zeros((3,), dtype=torch.int32, device="cuda"))):
        with pytest.raises(VidoError):
            bad()
    with pytest.raises(VidoError) as e:
        ops.mask_associate(m, c, s, hold=-1)
    assert e.value.code == -1
    with pytest.raises(VidoError) as e:
        ops.mask_associate(m, c, s, n=128)
    assert e.value.code == -4                                             # VIDO_E_CAPACITY
    with pytest.raises(VidoError) as e:
        ops.mask_associate(m, c, s, n=-1)
    assert e.value.code == -1
    big = torch.zeros((CTX_H + 1, CTX_W), dtype=torch.int32, device="cuda")
    with pytest.raises(VidoError) as e:
        ops.mask_associate(None, big, s)
    assert e.value.code == -1                                             # VIDO_E_INVALID, from the library
    # the C entry point itself
    ctx = ops.ctx; o = torch.empty_like(m)
    P = lambda t: C.c_void_p(t.data_ptr())
    call = lambda prev, cur, H, W, n, hold, state, out: ctx.lib.vido_mask_associate(ctx.h, prev, cur, H, W, None, n, hold, state, out, None, None)
    assert call(P(m), None, 64, 64, 1, 0, P(s), P(o)) == -1
    assert call(P(m), P(c), 64, 64, 1, 0, None, P(o)) == -1
    assert call(P(m), P(c), 64, 64, 1, 0, P(s), None) == -1
    assert call(P(m), P(c), 64, 64, 1, 0, P(s), P(m)) == -1
    assert call(P(m), P(c), 0, 64, 1, 0, P(s), P(o)) == -1
    assert call(P(m), P(c), 64, -1, 1, 0, P(s), P(o)) == -1
    assert call(P(m), P(c), 64, 64, 1, -1, P(s), P(o)) == -1
    assert call(P(m), P(c), 64, 64, -1, 0, P(s), P(o)) == -1
    assert call(P(m), P(c), 64, 64, 128, 0, P(s), P(o)) == -4
    assert call(None, P(c), 64, 64, 127, 0, P(s), P(c)) == 0              # no previous image, in place: fine
    torch.cuda.synchronize()
    assert not s.any().item()                                             # none of the refused calls touched the state
    assert not ops.mask_associate(m, c, s).any().item()
