"""MI355X: vido_mask_components / vido_frame_split_mask (csrc/maskcc.hip) against the numpy statement of the rule (tests/refimpl/mask_components_np.py): the instance image,
the per-component classes and areas and the four counters are EQUAL, on seeded blob images with hostile values and on the patterns where component labelling breaks
(tests/refimpl/cc_patterns.py: tile seams, corners, long chains, a flood of components), at five sizes, both connectivities, min_area 1 and 20; in place, 4-byte aligned
buffers, sizes back to back through one context, id base 127, graph replay, the tracker's slot call and the refusals.  Every reference is computed once (REF) and never
modified."""
import ctypes as C

import numpy as np
import pytest
import torch

from refimpl import cc_patterns as P
from refimpl.mask_components_np import components

pytestmark = pytest.mark.gpu

CTX_W, CTX_H = 1242, 375
SIZES = ((64, 64), (201, 151), (375, 1242), (1, 777), (777, 1))     # H, W
SMALL = SIZES[:2]                                                    # the long chains: the two smallest square-ish sizes only
PATTERNS = {"blobs": lambda H, W: P.blobs(H, W, 31 + H + W), "blobs2": lambda H, W: P.blobs(H, W, 977 + H), "full": P.full, "empty": P.empty, "checkerboard": P.checkerboard,
            "corner": P.corner_touch, "corner_anti": lambda H, W: P.corner_touch(H, W, anti=True), "spirals": P.spirals, "serpentine": P.serpentine, "comb": P.comb}
CHAINS = ("spirals", "serpentine", "comb")
CASES = [(name, H, W) for name in PATTERNS for (H, W) in (SMALL if name in CHAINS else SIZES)]
REF = {}


def image(name, H, W):
    key = ("img", name, H, W)
    if key not in REF:
        m = PATTERNS[name](H, W)
        m.setflags(write=False)
        REF[key] = m
    return REF[key]


def reference(name, H, W, conn, min_area=1, id_base=0, cap=127):
    """-> (mask, (out, classes, areas, stats)) of the numpy statement; computed once per argument set."""
    key = (name, H, W, conn, min_area, id_base, cap)
    if key not in REF:
        r = components(image(name, H, W), conn, min_area=min_area, id_base=id_base, cap=cap)
        for a in r:
            a.setflags(write=False)
        REF[key] = r
    return image(name, H, W), REF[key]


@pytest.fixture(scope="module")
def ops(vido):
    from vido_slam_amd import nets
    ctx = vido.Context(width=CTX_W, height=CTX_H, max_batch=1)
    yield nets.HipOps(ctx)
    torch.cuda.synchronize()
    ctx.close()


def dev(a, offset=0):
    """A device copy of `a` that starts `offset` elements behind an allocation's start (offset 1: 4-byte aligned only)."""
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    if offset:
        buf = torch.empty((t.numel() + offset,), dtype=t.dtype, device="cuda")
        v = buf[offset:].view(t.shape); v.copy_(t)
        return v
    return t


def run(ops, mask, conn, min_area=1, id_base=0, cap=127, alias=False, offsets=(0, 0)):
    """-> (out, classes, areas, stats) as numpy, every output pre-filled with garbage; the input is checked to be untouched"""
    tm = dev(mask, offsets[0])
    out = tm if alias else dev(np.full(mask.shape, -559038737, np.int32), offsets[1])
    cl = torch.full((cap,), -12345, dtype=torch.int64, device="cuda"); ar = torch.full((cap,), -12345, dtype=torch.int32, device="cuda")
    st = torch.full((4,), -12345, dtype=torch.int32, device="cuda")
    r = ops.mask_components(tm, connectivity=conn, min_area=min_area, id_base=id_base, cap=cap, out=out, classes=cl, areas=ar, stats=st)
    assert r is out
    torch.cuda.synchronize()
    if not alias:
        assert np.array_equal(tm.cpu().numpy(), mask)
    return out.cpu().numpy(), cl.cpu().numpy(), ar.cpu().numpy(), st.cpu().numpy()


def same(got, ref, what=""):
    for name, g, r in zip(("out", "classes", "areas", "stats"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), "%s %s: %d elements differ (stats %s, reference %s)" % (
            what, name, int((g != r).sum()), got[3].tolist(), ref[3].tolist())


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name,H,W", CASES)
def test_equal_to_the_numpy_statement(ops, name, H, W, conn):
    for min_area in (1, 20):
        mask, ref = reference(name, H, W, conn, min_area)
        got = run(ops, mask, conn, min_area)
        print("%s %dx%d conn %d min_area %d: stats %s, reference %s" % (name, H, W, conn, min_area, got[3].tolist(), ref[3].tolist()))
        same(got, ref, "min_area %d" % min_area)
    found = reference(name, H, W, conn, 1)[1][3]
    if name == "checkerboard" and conn == 4:
        assert found[2] > 0                                            # more components than the cap: left out
    if name.startswith("blobs") and H > 1 and W > 1:
        assert found[0] > 5 and reference(name, H, W, conn, 20)[1][3][1] > 0      # the case holds components, and some below 20 pixels


def test_in_place_and_4_byte_aligned_buffers(ops):
    H, W = 201, 151                                                    # an odd width and an odd pixel count: scalar head and tail
    for name, conn in (("blobs", 8), ("serpentine", 4)):
        mask, ref = reference(name, H, W, conn)
        same(run(ops, mask, conn, alias=True), ref, "out is mask")
        same(run(ops, mask, conn, offsets=(1, 1)), ref, "4-byte aligned, both alike")
        same(run(ops, mask, conn, offsets=(3, 2)), ref, "12 and 8 bytes off a boundary")
        same(run(ops, mask, conn, offsets=(0, 1)), ref, "out 4 bytes off")
        same(run(ops, mask, conn, alias=True, offsets=(3, 0)), ref, "in place, 12 bytes off")
    # a few pixels only: everything is head or tail
    for Hs, Ws in ((1, 1), (1, 3), (2, 3)):
        m = np.full((Hs, Ws), 7, np.int32)
        for off in (0, 1, 2, 3):
            same(run(ops, m, 8, offsets=(off, off)), components(m, 8), "%dx%d offset %d" % (Hs, Ws, off))


def test_different_sizes_back_to_back_through_one_context(ops):
    """A parent, an area or a row count left by the call before would show in the next result: large, small, large with other content, a column, a row, small again."""
    seq = (("checkerboard", 375, 1242, 4), ("blobs", 64, 64, 8), ("blobs", 375, 1242, 8), ("full", 777, 1, 4), ("blobs", 1, 777, 8), ("comb", 64, 64, 4), ("empty", 375, 1242, 8),
           ("blobs2", 201, 151, 4))
    for name, H, W, conn in seq:
        mask, ref = reference(name, H, W, conn)
        same(run(ops, mask, conn), ref, "%s %dx%d" % (name, H, W))


def test_id_base_127_and_a_small_cap(ops):
    H, W = 201, 151
    mask, ref = reference("blobs", H, W, 8, 1, 127, 127)
    got = run(ops, mask, 8, id_base=127)
    same(got, ref)
    assert got[0].max() == 127 + ref[3][3] and got[0][got[0] > 0].min() == 128
    mask, ref = reference("blobs", H, W, 8, 5, 250, 4)
    got = run(ops, mask, 8, min_area=5, id_base=250, cap=4)
    same(got, ref)
    assert ref[3][2] > 0 and got[0].max() == 254 and got[1].shape == (4,)
    same(run(ops, mask, 4, min_area=0, id_base=0, cap=1), components(mask, 4, 0, 0, 1))


def test_graph_replay_follows_the_input(ops):
    H, W = 201, 151
    cases = [reference(name, H, W, 8, 20) for name in ("blobs", "serpentine", "blobs2", "empty")]
    sm = torch.zeros((H, W), dtype=torch.int32, device="cuda"); so = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    sc = torch.zeros((127,), dtype=torch.int64, device="cuda"); sa = torch.zeros((127,), dtype=torch.int32, device="cuda"); ss = torch.zeros((4,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.mask_components(sm, min_area=20, out=so, classes=sc, areas=sa, stats=ss)      # the warm-up call: the planes exist before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mask_components(sm, min_area=20, out=so, classes=sc, areas=sa, stats=ss)
    for mask, ref in cases:
        sm.copy_(torch.from_numpy(mask.copy()))
        so.fill_(-7); sc.fill_(-7); sa.fill_(-7); ss.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        same((so.cpu().numpy(), sc.cpu().numpy(), sa.cpu().numpy(), ss.cpu().numpy()), ref, "replay")


def test_the_trackers_slot_call(vido):
    """vido_frame_split_mask: the slot's mask is split in place on the context's own stream; depth and flow of the slot are untouched."""
    from vido_slam_amd import host
    from vido_slam_amd.host import VidoError
    H, W = 240, 320
    ctx = vido.Context(width=W, height=H, max_batch=2)
    ff = host.FrameFeatures(ctx, host.track_params(dataset=1, fx=250.0, fy=250.0, cx=159.5, cy=119.5))
    m = P.blobs(H, W, 5)
    rng = np.random.RandomState(3)
    ff.upload(0, (1 + rng.rand(H, W)).astype(np.float32), rng.randn(H, W, 2).astype(np.float32), m)
    d0, f0, m0 = [a.copy() for a in ff.read_maps(0)]
    assert np.array_equal(m0.reshape(H, W), m)
    st = ctx.frame_split_mask(0, connectivity=8, min_area=20, id_base=127, cap=100)
    ref = components(m, 8, 20, 127, 100)
    d1, f1, m1 = ff.read_maps(0)
    assert np.array_equal(m1.reshape(H, W), ref[0]) and list(st) == ref[3].tolist() and st[3] > 0
    assert np.array_equal(d1, d0) and np.array_equal(f1, f0)
    for bad in (lambda: ctx.frame_split_mask(-1), lambda: ctx.frame_split_mask(2), lambda: ctx.frame_split_mask(0, connectivity=6),
                lambda: ctx.frame_split_mask(0, id_base=-1), lambda: ctx.frame_split_mask(0, cap=0)):
        with pytest.raises(VidoError) as e:
            bad()
        assert e.value.code == -1
    with pytest.raises(VidoError) as e:
        ctx.frame_split_mask(0, id_base=128, cap=127)
    assert e.value.code == -4
    assert np.array_equal(ff.read_maps(0)[2], m1)                     # none of the refused calls touched the slot
    ctx.close()


def test_refusals(ops):
    from vido_slam_amd.host import VidoError
    m = torch.zeros((64, 64), dtype=torch.int32, device="cuda"); o = torch.full((64, 64), 5, dtype=torch.int32, device="cuda")
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")
    for bad in (lambda: ops.mask_components(None), lambda: ops.mask_components(m.cpu()), lambda: ops.mask_components(m, out=o.cpu()),
                lambda: ops.mask_components(m.to(torch.int64)), lambda: ops.mask_components(m, out=o.to(torch.uint8)), lambda: ops.mask_components(m.t()),
                lambda: ops.mask_components(m.view(-1)), lambda: ops.mask_components(m, out=torch.zeros((64, 63), dtype=torch.int32, device="cuda")),
                lambda: ops.mask_components(m.view(-1)[:64 * 63].view(64, 63), out=m.view(-1)[4:4 + 64 * 63].view(64, 63)),      # out overlaps mask without being mask
                lambda: ops.mask_components(m, classes=i32(127)), lambda: ops.mask_components(m, classes=torch.zeros((126,), dtype=torch.int64, device="cuda")),
                lambda: ops.mask_components(m, areas=i32(126)), lambda: ops.mask_components(m, areas=torch.zeros((127,), dtype=torch.int64, device="cuda")),
                lambda: ops.mask_components(m, stats=i32(3)), lambda: ops.mask_components(m, stats=i32(4).cpu())):
        with pytest.raises(VidoError):
            bad()
    for kw, code in ((dict(connectivity=6), -1), (dict(connectivity=0), -1), (dict(id_base=-1), -1), (dict(cap=0), -1), (dict(cap=-3), -1),
                     (dict(id_base=128, cap=127), -4), (dict(id_base=0, cap=255), -4), (dict(id_base=254, cap=1), -4)):
        with pytest.raises(VidoError) as e:
            ops.mask_components(m, out=o, **kw)
        assert e.value.code == code, kw
    big = torch.zeros((CTX_H + 1, CTX_W), dtype=torch.int32, device="cuda")
    with pytest.raises(VidoError) as e:
        ops.mask_components(big)
    assert e.value.code == -1                                             # VIDO_E_INVALID, from the library
    # the C entry point itself
    ctx = ops.ctx
    Pt = lambda t: C.c_void_p(t.data_ptr())
    call = lambda mask, H, W, conn, ma, base, cap, out: ctx.lib.vido_mask_components(ctx.h, mask, H, W, conn, ma, base, cap, out, None, None, None)
    assert call(None, 64, 64, 8, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 64, 64, 8, 1, 0, 127, None) == -1
    assert call(Pt(m), 64, 63, 8, 1, 0, 127, C.c_void_p(m.data_ptr() + 16)) == -1
    assert call(Pt(m), 64, 64, 5, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 0, 64, 8, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 64, -1, 8, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 1, 4096, 8, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 4096, 1, 8, 1, 0, 127, Pt(o)) == -1
    assert call(Pt(m), 64, 64, 8, 1, -1, 127, Pt(o)) == -1
    assert call(Pt(m), 64, 64, 8, 1, 0, 0, Pt(o)) == -1
    assert call(Pt(m), 64, 64, 8, 1, 128, 127, Pt(o)) == -4
    torch.cuda.synchronize()
    assert bool((o == 5).all().item())                                    # none of the refused calls wrote the output
    assert call(Pt(m), 64, 64, 8, -7, 127, 127, Pt(m)) == 0               # in place, null per-component outputs, the last id base that fits: fine
    assert not ops.mask_components(m, out=o).any().item()
