"""GPU parity of the ORB front end on small and odd frames, on every input route and on batches with empty frames: bit-exact against the CPU oracle.

The extractor (csrc/orb.hip) picks its kernel forms from tables that build_tables lays out from the frame size: the tile grid of the single-launch pyramid, the
instantiation of k_fast_strips (interior 37 or 74), the rows a FAST strip holds, the blur strips per row, tiles or the k_resize chain.  The cases below are the
sizes at which those tables are tightest (one tile column, a 62-px top level, a single cell, one level, the widest cell interior and tallest strip an 8-level
pyramid reaches); each case first asserts from Context.orb_geometry() that the library really selected the forms it is there for (the expected values come from a
CPU restatement of build_tables' arithmetic), then compares every stage with oracle/orb_oracle.c.  Every comparison is np.array_equal."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave")
GEOM_FIELDS = ("n_levels", "n_ptiles", "nx", "ny", "fast_iw", "fast_rows", "max_interior", "n_strips", "n_cells", "n_blur_strips", "max_blur_row_strips", "slot_total")

# (width, height, scale, levels, n_features) -> the twelve fields of orb_geometry(), in GEOM_FIELDS order
CASES = [
    ((226, 226, 1.2, 8, 4000), (8, 10, 2, 5, 74, 59, 53, 52, 93, 75, 1, 23493)),      # widest interior (53) and tallest strip (59) of an 8-level pyramid; top level 63x63
    ((222, 222, 1.2, 8, 2000), (8, 10, 2, 5, 74, 57, 51, 52, 93, 72, 1, 22234)),      # top level exactly 62x62: a single FAST cell row and column
    ((223, 230, 1.2, 8, 500), (8, 10, 2, 5, 74, 46, 52, 53, 94, 75, 1, 23508)),       # odd widths on every level, budget far below the candidate count
    ((229, 517, 1.2, 8, 1000), (8, 22, 2, 11, 74, 44, 39, 142, 256, 161, 1, 64567)),  # portrait: 2x11 tiles, top level 64x144
    ((400, 225, 1.2, 8, 1000), (8, 20, 4, 5, 74, 58, 40, 97, 191, 111, 2, 47386)),    # two blur strips per row on three levels; 4x5 tiles
    ((250, 222, 1.2, 8, 1000), (8, 10, 2, 5, 74, 57, 46, 63, 100, 87, 2, 25604)),     # two blur strips on level 0 only (63 quads)
    ((121, 480, 1.1, 8, 1000), (8, 10, 1, 10, 74, 41, 53, 94, 119, 192, 1, 35843)),   # one tile column under ten rows; levels 121 .. 62 px wide
    ((109, 109, 1.2, 4, 300), (4, 2, 1, 2, 74, 59, 53, 5, 7, 26, 1, 2555)),           # one tile column, two tiles in all
    ((74, 100, 1.2, 2, 200), (2, 2, 1, 2, 37, 51, 36, 3, 3, 13, 1, 834)),             # two levels, narrow strips, level 1 is 62x83
    ((91, 91, 1.2, 1, 64), (1, 0, 0, 0, 74, 59, 53, 1, 1, 7, 1, 729)),                # one level: no pyramid launch at all, wide strips
    ((64, 64, 1.2, 1, 64), (1, 0, 0, 0, 37, 32, 26, 1, 1, 5, 1, 169)),                # the smallest frame vido_create accepts: one cell
    ((121, 97, 1.05, 9, 300), (9, 0, 0, 0, 74, 56, 52, 15, 19, 53, 1, 6356)),         # nine levels: no tiles are laid out, the k_resize chain on levels 121 .. 82 px wide (one resize tile column)
]
TOP_LEVEL = {(226, 226): (63, 63), (222, 222): (62, 62), (229, 517): (64, 144), (74, 100): (62, 83), (121, 480): (62, 246), (121, 97): (82, 66)}


def blocks_image(w, h, seed):
    """6x6-px blocks of two grey values (90 / 150) plus uniform noise 0..7, cropped to the frame."""
    rng = np.random.RandomState(seed)
    b = np.kron(rng.randint(0, 2, size=((h + 5) // 6, (w + 5) // 6)) * 60 + 90, np.ones((6, 6), np.int64))[:h, :w]
    return (b + rng.randint(0, 8, size=(h, w))).astype(np.uint8)


def noise_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)      # worst case: candidates everywhere


class Ref:
    """The oracle's stages for one gray image, computed once per (parameters, image) and never modified afterwards."""
    _cache = {}

    def __init__(self, oracle, p, gray):
        self.levels = oracle.orb_pyramid(p, gray)
        self.blurred = [oracle.gaussian_blur7(lv) for lv in self.levels]
        self.cands = [oracle.level_candidates(p, lv) for lv in self.levels]
        self.kps, self.desc, self.ncand = oracle.orb_extract(p, gray)
        for a in self.levels + self.blurred + [self.kps, self.desc]:
            a.setflags(write=False)

    @classmethod
    def get(cls, oracle, params, gray):
        nf, scale, levels = params
        key = (nf, scale, levels, gray.shape, gray.tobytes())
        if key not in cls._cache:
            cls._cache[key] = cls(oracle, oracle.orb_params(n_features=nf, scale_factor=scale, n_levels=levels), gray)
        return cls._cache[key]


def assert_textured(ref):
    """A condition on the INPUT, not on the kernel: the image must give the oracle candidates on every level, or the case tests nothing there."""
    assert all(n >= 1 for n in ref.ncand) and all(len(c[0]) >= 1 for c in ref.cands), ref.ncand


def check_candidates(ctx, f, ref):
    for l, (cx, cy, cr) in enumerate(ref.cands):
        gx, gy, gs = ctx.orb_candidates(f, l)
        assert len(gx) == len(cx) == ref.ncand[l], (f, l, len(gx), len(cx), ref.ncand[l])
        assert np.array_equal(gx - 16, cx.astype(np.int32)) and np.array_equal(gy - 16, cy.astype(np.int32)), (f, l)
        assert np.array_equal(gs, cr.astype(np.int32)), (f, l)


def check_stages(ctx, f, ref):
    for l, lv in enumerate(ref.levels):
        got = ctx.orb_level(f, l)
        assert got.shape == lv.shape, (f, l, got.shape, lv.shape)
        assert np.array_equal(got, lv), ("pyramid", f, l)
        assert np.array_equal(ctx.orb_level(f, l, blurred=True), ref.blurred[l]), ("blur", f, l)
    check_candidates(ctx, f, ref)


def check_result(k, d, ref, what=None, with_desc=True):
    assert len(k) == len(ref.kps), (what, len(k), len(ref.kps))
    for name in KP_FIELDS:
        assert np.array_equal(k[name], ref.kps[name]), (what, name)
    if with_desc:
        assert np.array_equal(d, ref.desc), what


def extract_raw(vido, ctx, ptr, on_device, n, frame_stride, stride, w, h):
    """vido_orb_extract_batch with every layout argument given; the descriptor array starts non-zero so that what comes back was written."""
    kps = np.zeros((n, ctx.max_kp), vido.KP_DTYPE); desc = np.full((n, ctx.max_kp, 32), 0xA5, np.uint8); cnt = np.full(n, -1, np.int32)
    ctx._check(ctx.lib.vido_orb_extract_batch(ctx.h, C.c_void_p(ptr), on_device, n, C.c_size_t(frame_stride), stride, w, h,
                                              kps.ctypes.data_as(C.c_void_p), ctx.max_kp, cnt.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p)))
    return kps, desc, cnt


def check_batch(kps, desc, cnt, refs, what, with_desc=True):
    assert len(cnt) == len(refs)
    for f, ref in enumerate(refs):
        check_result(kps[f, :cnt[f]], desc[f, :cnt[f]] if with_desc else None, ref, (what, f), with_desc)


def padded(frames, stride, frame_stride, lead=0, fill=255):
    """frames (n,h,wb) u8 laid out with rows `stride` and frames `frame_stride` bytes apart, `lead` bytes in front; every byte that is no pixel holds `fill`."""
    n, h, wb = frames.shape
    buf = np.full(lead + n * frame_stride + 16, fill, np.uint8)
    for f in range(n):
        rows = np.lib.stride_tricks.as_strided(buf[lead + f * frame_stride:], shape=(h, wb), strides=(stride, 1))
        rows[:] = frames[f]
    return buf


# ---- a) geometry sweep ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,forms", CASES, ids=["%dx%d_s%g_L%d_n%d" % c for c, _ in CASES])
def test_geometry_sweep(vido, oracle, case, forms):
    w, h, scale, levels, nf = case
    c = vido.Context(width=w, height=h, max_batch=2, n_features=nf, scale_factor=scale, n_levels=levels)
    try:
        g = c.orb_geometry()
        print("orb_geometry %s: %s" % (case, g))
        assert tuple(g) == GEOM_FIELDS
        assert g == dict(zip(GEOM_FIELDS, forms)), (case, g)
        assert c.orb_geometry() == g                                           # a read: asking again changes nothing
        params = (nf, scale, levels)
        imgs = np.stack([blocks_image(w, h, 3), blocks_image(w, h, 4)])
        refs = [Ref.get(oracle, params, im) for im in imgs]
        if (w, h) in TOP_LEVEL:
            assert refs[0].levels[-1].shape == TOP_LEVEL[(w, h)][::-1]
        for r in refs:
            assert_textured(r)
        kps, desc, cnt = c.orb_extract_batch(imgs)
        for f in range(2):
            check_stages(c, f, refs[f])
        check_batch(kps, desc, cnt, refs, "blocks")
        noise = noise_image(w, h, 1)
        rn = Ref.get(oracle, params, noise)
        k, d = c.orb_extract(noise)
        check_candidates(c, 0, rn)
        check_result(k, d, rn, "noise")
        assert c.orb_geometry() == g
    finally:
        c.close()


def test_sweep_covers_every_form():
    """What the sweep is for: both strip instantiations, one and several tile columns, with and without a tile launch, one and two blur strips per row, and the
    widest interior together with the tallest strip (each case asserts its row from orb_geometry() above)."""
    rows = [dict(zip(GEOM_FIELDS, f)) for _, f in CASES]
    assert {r["fast_iw"] for r in rows} == {37, 74}
    assert any(r["nx"] == 1 and r["n_ptiles"] > 0 for r in rows) and any(r["nx"] > 1 for r in rows)
    assert any(r["n_ptiles"] == 0 for r in rows) and any(r["n_ptiles"] > 0 for r in rows)
    assert {r["max_blur_row_strips"] for r in rows} == {1, 2}
    assert any(r["max_interior"] == 53 and r["fast_rows"] >= 59 for r in rows)
    assert all(r["n_ptiles"] in (0, r["nx"] * r["ny"]) for r in rows)


# ---- b) input routes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(226, 226), (223, 230)], ids=["226x226", "223x230"])
def test_gray_input_routes(vido, oracle, size):
    """Every way a gray frame can reach level 0 gives the contiguous host call's result: a padded host frame (2-D copy), a device frame that is no multiple of 4 wide
    (k_ingest), a 228-wide aligned device frame (ingest fused into the tile launch), the same frame at an odd address and stride (k_ingest again), frames further apart
    than stride x height."""
    import torch
    w, h = size
    params = (1000, 1.2, 8)
    for cw in (w, 228):
        c = vido.Context(width=cw, height=h, max_batch=2, n_features=1000)
        try:
            assert c.orb_geometry()["n_ptiles"] == 10                          # the tile launch exists: whether the ingest rides on it is decided per call
            imgs = np.stack([blocks_image(cw, h, 3), blocks_image(cw, h, 4)])
            refs = [Ref.get(oracle, params, im) for im in imgs]
            base = c.orb_extract_batch(imgs)                                   # the contiguous host call
            check_batch(*base, refs, ("host", cw))

            def same(got, what, n=2):
                kps, desc, cnt = got
                assert np.array_equal(cnt, base[2][:n]), (what, cnt, base[2])
                for f in range(n):
                    m = cnt[f]
                    assert np.array_equal(kps[f, :m], base[0][f, :m]) and np.array_equal(desc[f, :m], base[1][f, :m]), (what, f)
                    assert np.array_equal(c.orb_level(f, 0), imgs[f]), (what, f)          # level 0 holds the pixels and nothing of the padding
                    check_stages(c, f, refs[f])

            # host, stride = width + 13, pad bytes 255; then frames 37 bytes further apart than stride x height as well
            st = cw + 13
            buf = padded(imgs, st, st * h)
            same(extract_raw(vido, c, buf.ctypes.data, 0, 2, st * h, st, cw, h), "host stride")
            k1 = np.zeros(c.max_kp, vido.KP_DTYPE); d1 = np.zeros((c.max_kp, 32), np.uint8); n1 = C.c_int()
            c._check(c.lib.vido_orb_extract(c.h, C.c_void_p(buf.ctypes.data + st * h), st, cw, h, k1.ctypes.data_as(C.c_void_p), c.max_kp, C.byref(n1), d1.ctypes.data_as(C.c_void_p)))
            check_result(k1[:n1.value], d1[:n1.value], refs[1], "single host frame, stride")
            buf = padded(imgs, st, st * h + 37)
            same(extract_raw(vido, c, buf.ctypes.data, 0, 2, st * h + 37, st, cw, h), "host frame_stride")
            # device, contiguous: fused ingest when the width is a multiple of 4 (228), k_ingest otherwise
            dev = torch.from_numpy(imgs).cuda()
            assert dev.data_ptr() % 4 == 0
            same(c.orb_extract_batch((dev.data_ptr(), 2, h, cw, h * cw, cw)), "device contiguous")
            same(extract_raw(vido, c, dev.data_ptr(), 1, 1, h * cw, cw, cw, h), "device one frame", n=1)
            # device, frames a multiple of 4 further apart (still fused at 228) and an odd amount further apart (k_ingest)
            for extra in (64, 37):
                dbuf = torch.from_numpy(padded(imgs, cw, cw * h + extra)).cuda()
                same(extract_raw(vido, c, dbuf.data_ptr(), 1, 2, cw * h + extra, cw, cw, h), ("device frame_stride", extra))
            # device, one byte into the allocation with stride = width + 3: no dword loads possible
            dbuf = torch.from_numpy(padded(imgs, cw + 3, (cw + 3) * h, lead=1)).cuda()
            assert dbuf.data_ptr() % 4 == 0
            same(extract_raw(vido, c, dbuf.data_ptr() + 1, 1, 2, (cw + 3) * h, cw + 3, cw, h), "device odd address and stride")
            torch.cuda.synchronize()
        finally:
            c.close()


@pytest.mark.parametrize("size", [(226, 226), (223, 230)], ids=["226x226", "223x230"])
def test_colour_input_routes(vido, oracle, size):
    """3- and 4-channel frames in both channel orders with a padded stride, from the host and from the device: the returned gray image equals the oracle's cvtColor
    and the extraction equals the oracle's on that gray image."""
    import torch
    w, h = size
    params = (1000, 1.2, 8)
    c = vido.Context(width=w, height=h, max_batch=2, n_features=1000)
    try:
        for cn in (3, 4):
            col = np.stack([np.stack([blocks_image(w, h, 10 * f + 3 + ch) for ch in range(cn)], axis=-1) for f in range(2)])      # (2, h, w, cn), channels independent
            st = w * cn + 13
            fs = st * h + 29
            buf = padded(col.reshape(2, h, w * cn), st, fs)
            dbuf = torch.from_numpy(buf).cuda()
            for rgb in (0, 1):
                grays = [oracle.bgr2gray(col[f], rgb_order=bool(rgb)) for f in range(2)]
                refs = [Ref.get(oracle, params, g) for g in grays]
                for r in refs:
                    assert_textured(r)
                for on_device in (0, 1):
                    what = (cn, rgb, on_device)
                    kps = np.zeros((2, c.max_kp), vido.KP_DTYPE); desc = np.full((2, c.max_kp, 32), 0xA5, np.uint8); cnt = np.full(2, -1, np.int32)
                    if on_device:
                        gdev = torch.full((2 * h * w + 16,), 0x5A, dtype=torch.uint8, device="cuda"); src, gptr = dbuf.data_ptr(), gdev.data_ptr()
                    else:
                        ghost = np.full(2 * h * w + 16, 0x5A, np.uint8); src, gptr = buf.ctypes.data, ghost.ctypes.data
                    c._check(c.lib.vido_orb_extract_color(c.h, C.c_void_p(src), cn, rgb, on_device, 2, C.c_size_t(fs), st, w, h, C.c_void_p(gptr),
                                                          kps.ctypes.data_as(C.c_void_p), c.max_kp, cnt.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p)))
                    if on_device:
                        torch.cuda.synchronize(); ghost = gdev.cpu().numpy()
                    assert np.array_equal(ghost[:2 * h * w].reshape(2, h, w), np.stack(grays)), what
                    assert (ghost[2 * h * w:] == 0x5A).all(), what                 # nothing written past the two tight images
                    for f in range(2):
                        assert np.array_equal(c.orb_level(f, 0), grays[f]), (what, f)
                        check_candidates(c, f, refs[f])
                    check_batch(kps, desc, cnt, refs, what)
    finally:
        c.close()


# ---- c) batches -----------------------------------------------------------------------------------------------------------------------------------------
def test_batches_with_empty_frames(vido, oracle):
    """Prefixes of nine frames (flat, blocks, blocks, noise, flat, blocks, flat, blocks, flat) at 226x226: one frame (lean, k_scan_counts), two (lean, per-frame scans),
    three (forked blur), eight and nine (orientation + rBRIEF in two launches, an empty frame at the head of each half and at the tail).  Counts and every row equal the
    per-frame oracle, and a two-frame call after the nine-frame one meets stale rows and counts of the larger batch."""
    w = h = 226
    params = (1000, 1.2, 8)
    flat = np.full((h, w), 77, np.uint8)
    frames = np.stack([flat, blocks_image(w, h, 3), blocks_image(w, h, 4), noise_image(w, h, 1), flat, blocks_image(w, h, 5), flat, blocks_image(w, h, 6), flat])
    refs = [Ref.get(oracle, params, g) for g in frames]
    for f in (1, 2, 3, 5, 7):
        assert_textured(refs[f])
    for f in (0, 4, 6, 8):
        assert len(refs[f].kps) == 0 and sum(refs[f].ncand) == 0
    c = vido.Context(width=w, height=h, max_batch=9, n_features=1000)
    try:
        for n in (1, 2, 3, 8, 9, 2):
            kps, desc, cnt = c.orb_extract_batch(frames[:n])
            assert cnt.tolist() == [len(r.kps) for r in refs[:n]], (n, cnt)
            assert all(cnt[f] == 0 for f in (0, 4, 6, 8) if f < n)
            check_batch(kps, desc, cnt, refs[:n], n)
            if n == 9:
                for f in (3, 8):
                    check_candidates(c, f, refs[f])
            else:
                check_candidates(c, n - 1, refs[n - 1])
        k, d = c.orb_extract(frames[5])                                        # and the single-frame entry after the batches
        check_result(k, d, refs[5], "single after batches")
    finally:
        c.close()


def test_fused_front_end_mirrors_both_halves(vido, oracle):
    """vido_frontend_batch hands the extractor's rows back through the pinned mirror: from eight frames on the first half's rows leave on the second stream while the
    second half is still being computed.  The same nine frames, then eight, then two (rows of the larger batches still in the mirror): every row equals the oracle's."""
    w = h = 226
    params = (1000, 1.2, 8)
    flat = np.full((h, w), 77, np.uint8)
    frames = np.stack([flat, blocks_image(w, h, 3), blocks_image(w, h, 4), noise_image(w, h, 1), flat, blocks_image(w, h, 5), flat, blocks_image(w, h, 6), flat])
    refs = [Ref.get(oracle, params, g) for g in frames]
    c = vido.Context(width=w, height=h, max_batch=9, n_features=1000)
    try:
        ff = vido.FrameFeatures(c, vido.track_params(dataset=0, depth_map_factor=1.0, th_depth_bg=40.0, th_depth_obj=25.0, cx=w / 2, cy=h / 2))
        for n in (9, 8, 2):
            depth = np.full((n, h, w), 2.0, np.float32); flow = np.zeros((n, h, w, 2), np.float32); mask = np.zeros((n, h, w), np.int32)
            out = ff.frontend_batch(0, frames[:n], depth, flow, mask)
            assert out["n_kp"].tolist() == [len(r.kps) for r in refs[:n]], (n, out["n_kp"])
            check_batch(out["kps"], out["desc"], out["n_kp"], refs[:n], ("frontend", n))
    finally:
        c.close()


# ---- d) no descriptors ----------------------------------------------------------------------------------------------------------------------------------
def test_without_descriptors(vido, oracle):
    w, h = 223, 230
    params = (1000, 1.2, 8)
    frames = np.stack([blocks_image(w, h, 3), noise_image(w, h, 1), blocks_image(w, h, 4)])
    refs = [Ref.get(oracle, params, g) for g in frames]
    c = vido.Context(width=w, height=h, max_batch=3, n_features=1000, compute_descriptors=0)
    try:
        kps, desc, cnt = extract_raw(vido, c, frames.ctypes.data, 0, 3, w * h, w, w, h)
        check_batch(kps, desc, cnt, refs, "no descriptors", with_desc=False)      # angle included
        for f in range(3):
            assert cnt[f] > 0 and not desc[f, :cnt[f]].any(), f                # the descriptor output is zero
            check_candidates(c, f, refs[f])
        with pytest.raises(vido.VidoError) as e:
            c.orb_describe_points(0, np.array([[100, 100, 0]], np.int32))
        assert e.value.code == -1 and "compute_descriptors" in str(e.value)
    finally:
        c.close()


# ---- e) refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refused_sizes_then_the_smallest_context(vido, oracle):
    for kw, word in ((dict(width=64, height=64, n_levels=2), "level 1 is 53x53"), (dict(width=74, height=64, n_levels=2), "level 1 is 62x53"), (dict(width=63, height=64, n_levels=1), "63x64")):
        with pytest.raises(vido.VidoError) as e:
            vido.Context(max_batch=1, n_features=64, **kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    try:
        g = blocks_image(64, 64, 5)
        ref = Ref.get(oracle, (64, 1.2, 1), g)
        assert_textured(ref)
        k, d = c.orb_extract(g)
        check_stages(c, 0, ref)
        check_result(k, d, ref, "64x64")
    finally:
        c.close()
