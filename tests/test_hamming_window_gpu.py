"""MI355X: vido_hamming_match_window (csrc/hamwin.hip) against the numpy statement of the rule (tests/refimpl/hamming_window_np.py): all five outputs bit-exact over
the sizes at which the kernel changes path (queries per wave 4, per workgroup 16; train chunk 512), both radii, every level gate, max_dist, ratio and unique setting,
points exactly on the window's edge, NaN / inf positions, 50 queries claiming one train entry, a permuted train set, the device-pointer form, the refusals and one case
of the tracker's size.  Descriptors come from a few families of near-duplicates (exact copies included) so that small distances, ties and duplicates are the rule;
positions lie on a 64 x 64 px field in steps of 0.5 px.  Every reference is computed once (REF) and never modified."""
import numpy as np
import pytest
import torch

from refimpl.hamming_window_np import match_window

pytestmark = pytest.mark.gpu

CHUNK = 512                                     # HW_CH of csrc/hamwin.hip
NQS = (0, 1, 7, 8, 9, 33, 257)
NTS = (0, 1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
CONFIGS = (dict(radius=3.5, level_tol=1, max_dist=256, ratio=None, unique=False),
           dict(radius=3.5, level_tol=0, max_dist=256, ratio=(819, 1024), unique=True),
           dict(radius=0.0, level_tol=-1, max_dist=0, ratio=(1, 1), unique=True),
           dict(radius=3.5, level_tol=-1, max_dist=40, ratio=(1, 1), unique=False))
REF = {}


def make(nq, nt, seed, field=64, step=0.5):
    """Queries and train entries: descriptors = one of 24 base descriptors with 0 .. 8 random bits flipped (0 flips: exact duplicates); positions on the field in
    multiples of `step`; a third of the train entries sit exactly on a query's position (radius 0 finds them); levels 0 .. 3."""
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, (24, 32), dtype=np.uint8)

    def fam(n):
        d = base[r.integers(0, 24, n)].copy()
        for i in range(n):
            for b in r.integers(0, 256, r.integers(0, 9)):
                d[i, b // 8] ^= np.uint8(1 << (b % 8))
        return d
    qd, td = fam(nq), fam(nt)
    qxy = (r.integers(0, int(field / step), (nq, 2)) * step).astype(np.float32); txy = (r.integers(0, int(field / step), (nt, 2)) * step).astype(np.float32)
    if nq and nt:
        on = np.flatnonzero(r.random(nt) < 0.33)
        txy[on] = qxy[r.integers(0, nq, len(on))]
    ql = r.integers(0, 4, nq).astype(np.int32); tl = r.integers(0, 4, nt).astype(np.int32)
    return qd, qxy, ql, td, txy, tl


def reference(key, inputs, **cfg):
    if key not in REF:
        REF[key] = match_window(*inputs, **cfg)
        for a in REF[key]:
            a.setflags(write=False)
    return REF[key]


def same(got, want, what=""):
    for name, a, b in zip(("idx", "dist", "dist2", "status", "stats"), got, want):
        assert a.dtype == np.int32 and np.array_equal(a, b), (what, name, np.flatnonzero(np.asarray(a) != np.asarray(b))[:8])


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=640, height=480, max_batch=1)
    yield c
    c.close()


@pytest.mark.parametrize("nt", NTS)
def test_bit_exact_over_sizes_and_settings(ctx, nt):
    seen = set()
    for nq in NQS:
        inputs = make(nq, nt, 1000 * nt + nq)
        for ci, cfg in enumerate(CONFIGS):
            want = reference(("sizes", nq, nt, ci), inputs, **cfg)
            same(ctx.hamming_match_window(*inputs, **cfg), want, (nq, nt, cfg))
            seen |= set(want[3].tolist())
    if nt >= 63:
        assert seen >= {0, 1, 2, 3}, seen                    # every verdict occurs at this train size (lost claims: at the smaller ones, and in the tests below)


def test_windows_hold_zero_to_about_twenty_candidates():
    """The premise of the sizes above, counted on the CPU: at the largest train set the windows of radius 3.5 hold from none to a few tens of candidates."""
    qd, qxy, ql, td, txy, tl = make(257, 2 * CHUNK + 3, 7)
    n = ((np.abs(txy[None, :, 0] - qxy[:, None, 0]) <= 3.5) & (np.abs(txy[None, :, 1] - qxy[:, None, 1]) <= 3.5)).sum(1)
    assert n.min() <= 4 and 10 <= np.median(n) <= 30 and n.max() <= 60, (n.min(), np.median(n), n.max())


def test_points_exactly_on_the_edge(ctx):
    """Positions in steps of 0.25 px and a radius of 2.25: many pairs sit exactly on the window's edge (|dx| == radius), which is inside; one ulp less radius loses them."""
    inputs = make(257, CHUNK + 1, 11, field=24, step=0.25)
    qxy, txy = inputs[1], inputs[4]
    dx = np.abs(txy[None, :, 0] - qxy[:, None, 0]); dy = np.abs(txy[None, :, 1] - qxy[:, None, 1])
    edge = ((dx == 2.25) & (dy <= 2.25)) | ((dy == 2.25) & (dx <= 2.25))
    assert edge.sum() > 500
    cfg = dict(level_tol=-1, max_dist=256, ratio=None, unique=False)
    inside = reference(("edge", 0), inputs, radius=2.25, **cfg)
    below = reference(("edge", 1), inputs, radius=float(np.nextafter(np.float32(2.25), np.float32(0))), **cfg)
    assert (inside[1] != below[1]).sum() > 20                # the edge entries decide some bests
    same(ctx.hamming_match_window(*inputs, radius=2.25, **cfg), inside)
    same(ctx.hamming_match_window(*inputs, radius=float(np.nextafter(np.float32(2.25), np.float32(0))), **cfg), below)


def test_fifty_queries_claim_one_train_entry(ctx):
    """Train entry 3 is the best of all 50 queries (the query = that descriptor with 1 + i % 7 bits flipped, so distances repeat); the other train entries are in the window
    but far in descriptor space.  The smallest (dist, i) keeps the entry — query 0 at distance 1 — and the 49 others get status 4, not their second candidate."""
    r = np.random.default_rng(3)
    td = r.integers(0, 256, (40, 32), dtype=np.uint8); txy = np.full((40, 2), 5.0, np.float32); tl = np.zeros(40, np.int32)
    qd = np.repeat(td[3:4], 50, 0)
    for i in range(50):
        for b in range(1 + i % 7):
            qd[i, (7 * i + b) % 32] ^= np.uint8(1 << (b % 8))
    qxy = np.full((50, 2), 5.0, np.float32); ql = np.zeros(50, np.int32)
    want = reference("claim", (qd, qxy, ql, td, txy, tl), radius=1.0, level_tol=0, max_dist=256, ratio=None, unique=True)
    assert want[1].tolist() == [1 + i % 7 for i in range(50)] and (want[2] > 60).all()
    assert want[3].tolist() == [0] + [4] * 49 and want[0].tolist() == [3] + [-1] * 49 and want[4].tolist() == [1, 0, 0, 0, 49]
    same(ctx.hamming_match_window(qd, qxy, ql, td, txy, tl, 1.0, level_tol=0, max_dist=256, ratio=None, unique=True), want)
    # reversed query order: the winner is now the FIRST of the queries at distance 1 in the new order
    rev = reference("claim-rev", (qd[::-1].copy(), qxy, ql, td, txy, tl), radius=1.0, level_tol=0, max_dist=256, ratio=None, unique=True)
    assert rev[3].tolist().count(0) == 1 and rev[1][rev[3] == 0].tolist() == [1] and int(np.flatnonzero(rev[3] == 0)[0]) == int(np.flatnonzero(rev[1] == 1)[0])
    same(ctx.hamming_match_window(qd[::-1].copy(), qxy, ql, td, txy, tl, 1.0, level_tol=0, max_dist=256, ratio=None, unique=True), rev)


def test_nan_and_inf_positions(ctx):
    qd, qxy, ql, td, txy, tl = make(33, 65, 21)
    qxy = qxy.copy(); txy = txy.copy()
    qxy[4, 0] = np.nan; qxy[9, 1] = np.inf; qxy[17] = (-np.inf, np.nan); txy[5, 1] = np.nan; txy[40, 0] = np.inf
    for radius in (3.5, 1e30):
        want = reference(("nan", radius), (qd, qxy, ql, td, txy, tl), radius=radius, level_tol=-1, max_dist=256, ratio=None, unique=True)
        assert want[3][[4, 9, 17]].tolist() == [1, 1, 1] and not np.isin(want[0], (5, 40)).any()
        same(ctx.hamming_match_window(qd, qxy, ql, td, txy, tl, radius, level_tol=-1, max_dist=256, ratio=None, unique=True), want, radius)


def test_invariant_under_a_permutation_of_the_train_set(ctx):
    """Queries whose smallest candidate distance is reached twice are left out (the lowest-index rule is not what is being permuted; the claim's tie rule is over query
    indices, which stay); then a shuffled train set gives the same distances, verdicts and counters, and the same train entries once the indices are mapped back."""
    qd, qxy, ql, td, txy, tl = make(257, 2 * CHUNK + 3, 31)
    cfg = dict(radius=3.5, level_tol=1, max_dist=256, ratio=(922, 1024), unique=True)
    q = (qd, qxy, ql)
    ok = (np.abs(txy[None, :, 0] - q[1][:, None, 0]) <= 3.5) & (np.abs(txy[None, :, 1] - q[1][:, None, 1]) <= 3.5) & (np.abs(tl[None, :] - q[2][:, None]) <= 1)
    pop = np.array([bin(v).count("1") for v in range(256)], np.int32)
    D = np.where(ok, pop[q[0][:, None, :] ^ td[None, :, :]].sum(2), 999)
    untied = (D == D.min(1, keepdims=True)).sum(1) == 1
    q = tuple(a[untied] for a in q); assert len(q[0]) > 100
    want = reference("perm", q + (td, txy, tl), **cfg)
    assert set(want[3].tolist()) >= {0, 3, 4}
    same(ctx.hamming_match_window(*q, td, txy, tl, **cfg), want)
    perm = np.random.default_rng(9).permutation(len(td))
    got = ctx.hamming_match_window(*q, td[perm], txy[perm], tl[perm], **cfg)
    back = np.where(got[0] >= 0, perm[np.maximum(got[0], 0)], -1).astype(np.int32)
    same((back,) + tuple(got[1:]), want)


def test_device_form_equals_host_form(ctx):
    inputs = make(257, 2 * CHUNK + 3, 41)
    cfg = dict(radius=3.5, level_tol=1, max_dist=60, ratio=(819, 1024), unique=True)
    want = reference("device", inputs, **cfg)
    same(ctx.hamming_match_window(*inputs, **cfg), want)
    t = [torch.from_numpy(a.copy()).cuda() for a in inputs]
    nq, nt = len(inputs[0]), len(inputs[3])
    out = [torch.full((nq,), -559038737, dtype=torch.int32, device="cuda") for _ in range(4)]; st = torch.full((5,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for unique in (True, False):
        c = dict(cfg, unique=unique)
        ctx.hamming_match_window_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), nq, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), nt, c["radius"], c["level_tol"],
                                        c["max_dist"], c["ratio"], c["unique"], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), st.data_ptr())
        ctx.synchronize()
        same([o.cpu().numpy() for o in out] + [st.cpu().numpy()], reference(("device", unique), inputs, **c), unique)
    # without a counter array; and no query at all: the counters alone are written (zeros)
    for o in out:
        o.fill_(-7)
    torch.cuda.synchronize()
    ctx.hamming_match_window_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), nq, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), nt, cfg["radius"], cfg["level_tol"],
                                    cfg["max_dist"], cfg["ratio"], True, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None)
    ctx.synchronize()
    same([o.cpu().numpy() for o in out], want[:4])
    st.fill_(99); torch.cuda.synchronize()
    ctx.hamming_match_window_device(None, None, None, 0, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), nt, 3.5, 1, 60, None, True, None, None, None, None, st.data_ptr())
    ctx.synchronize()
    assert st.cpu().tolist() == [0] * 5


def test_refusals(ctx, vido):
    inputs = make(8, 9, 51)
    for ratio in ((2, 1), (1, 1025), (-1, 4), (1025, 1025), (5, 4)):
        with pytest.raises(vido.VidoError) as e:
            ctx.hamming_match_window(*inputs, radius=1.0, ratio=ratio)
        assert e.value.code == -1, ratio
    for radius in (-1.0, float("nan"), float("inf")):
        with pytest.raises(vido.VidoError) as e:
            ctx.hamming_match_window(*inputs, radius=radius)
        assert e.value.code == -1, radius
    # a ratio as a float is round(1024 r) / 1024; 0 and None switch the test off
    a = ctx.hamming_match_window(*inputs, radius=64.0, level_tol=-1, ratio=0.8); b = ctx.hamming_match_window(*inputs, radius=64.0, level_tol=-1, ratio=(819, 1024))
    same(a, b)
    same(ctx.hamming_match_window(*inputs, radius=64.0, level_tol=-1, ratio=0), ctx.hamming_match_window(*inputs, radius=64.0, level_tol=-1, ratio=None))


def test_the_trackers_size(ctx):
    inputs = make(3000, 2500, 61)
    cfg = dict(radius=1.5, level_tol=1, max_dist=10, ratio=(922, 1024), unique=True)
    want = reference("tracker", inputs, **cfg)
    assert min(want[4].tolist()) >= 10                       # every status occurs
    same(ctx.hamming_match_window(*inputs, **cfg), want)
