"""MI355X: the context's one host staging buffer (csrc/ctx.cpp: staging_upload / staging_download) shared by the host forms of different ops and sizes.  One Context, the
host forms back to back in an order that makes the buffer grow (dis_flow 64 x 48), be reused by smaller calls of other ops (stereo_filter 24 x 16, orb_patch_search with 3
points, flow_consistency 40 x 32), grow again (dis_flow_pair 96 x 80) and be reused again (hamming_match_window 5 x 70, stereo_sgm 16 x 16, dis_flow 64 x 48 once more).
Every result is bit-equal to the op's numpy statement in tests/refimpl/ on the same inputs, and the second dis_flow to the first.  Then one call per op family with some
outputs NULL, straight through the C entry points: the outputs asked for are unchanged and arrays that were not passed stay untouched."""
import ctypes as C
import numpy as np
import pytest

from refimpl import dis_flow_np as D
from refimpl import flow_consistency_np as F
from refimpl import flow_consistency_cases as FK
from refimpl import patch_search_np as PS
from refimpl import stereo_cases as SK
from refimpl import stereo_filter_cases as SFK
from refimpl import stereo_filter_np as SF
from refimpl import stereo_sgm_np as G
from refimpl.hamming_window_np import match_window
from test_dis_flow_gpu import _pair
from test_hamming_window_gpu import make

pytestmark = pytest.mark.gpu

HAM = dict(radius=3.5, level_tol=1, max_dist=64, ratio=(4, 5), unique=True)
SEARCH = dict(excl=2, min_var=4096, min_zncc_q10=920, peak_ratio_q10=900)


@pytest.fixture(scope="module")
def ctx(vido):
    c = vido.Context(width=64, height=64, max_batch=1, n_features=64, n_levels=1)
    c.orb_extract(vido.synth.make_frame(64, 64, seed=31))                                     # the frame orb_patch_search reads
    yield c
    c.close()


def _same(what, got, want):
    assert len(got) == len(want), what
    for k, (g, w_) in enumerate(zip(got, want)):
        if w_ is None:
            assert g is None, (what, k)
            continue
        g, w_ = np.asarray(g), np.asarray(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k)
        if g.dtype == np.float32:
            g, w_ = g.view(np.uint32), w_.view(np.uint32)                                     # NaNs compare by their bits
        assert np.array_equal(g, w_), (what, k, np.argwhere(g != w_)[:6].tolist())


@pytest.fixture(scope="module")
def inputs(vido, ctx):
    level = ctx.orb_level(0, 0, blurred=True)
    xyl = np.array([[20, 20, 0], [40, 30, 0], [-20, 2, 0]], np.int32)                         # two searched points and one outside the level
    ref = np.stack([level[17:25, 18:26].reshape(64), level[26:34, 37:45].reshape(64), level[0:8, 0:8].reshape(64)])
    return dict(dis=_pair(vido, 64, 48, seed=5), filt=SFK.random_case(16, 24, seed=3), level=level, xyl=xyl, ref=np.ascontiguousarray(ref),
                check=FK.random_fields(32, 40, seed=7), pair=_pair(vido, 96, 80, seed=6), ham=make(5, 70, seed=6), sgm=SK.warped_pair(16, 16, 16, seed=4))


def test_one_buffer_serves_every_op_in_turn(ctx, inputs):
    I = inputs
    first = ctx.dis_flow(*I["dis"], coarsest=2)                                               # grows
    _same("dis_flow 64 x 48", first, D.dis_flow(*I["dis"], coarsest=2))
    assert first[2][0] > 0 and first[1].any()
    with np.errstate(over="ignore"):
        want = SF.stereo_filter(*I["filt"], max_diff_q4=8, min_region=6, bf=75.0)
    _same("stereo_filter 24 x 16", ctx.stereo_filter(*I["filt"], max_diff_q4=8, min_region=6, bf=75.0), want)      # a smaller call of another op
    want = PS.patch_search([I["level"]], I["xyl"], I["ref"], 3, SEARCH["excl"], SEARCH["min_var"], SEARCH["min_zncc_q10"], SEARCH["peak_ratio_q10"])
    assert want[3][2] == -1 and (want[3][:2] >= 0).all()
    _same("orb_patch_search 3 points", ctx.orb_patch_search(0, I["xyl"], I["ref"], 3, **SEARCH), want)
    _same("flow_consistency 40 x 32", ctx.flow_consistency(*I["check"]), F.flow_consistency(*I["check"]))
    a, b = I["pair"]
    f, g = D.dis_flow(a, b, coarsest=2), D.dis_flow(b, a, coarsest=2)
    status, marked, cstats = F.flow_consistency(f[1], g[1])
    want = (marked, f[1], g[1], status, np.concatenate([f[2], g[2], cstats]).astype(np.int32))
    _same("dis_flow_pair 96 x 80", ctx.dis_flow_pair(a, b, coarsest=2), want)                 # grows again
    _same("hamming_match_window 5 x 70", ctx.hamming_match_window(*I["ham"], **HAM), match_window(*I["ham"], **HAM))
    _same("stereo_sgm 16 x 16", ctx.stereo_sgm(*I["sgm"], max_disp=16), G.stereo_sgm(*I["sgm"], max_disp=16))
    _same("dis_flow 64 x 48 again", ctx.dis_flow(*I["dis"], coarsest=2), first)


def test_null_outputs_take_no_copy(ctx, inputs):
    I = inputs; lib = ctx.lib
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    SENT = 0x5A
    def blank(like):
        return [np.frombuffer(bytes([SENT]) * a.nbytes, a.dtype).reshape(a.shape).copy() for a in like]
    def check(what, full, got, asked):
        for k, (w_, g) in enumerate(zip(full, got)):
            if k in asked:
                _same(what, (g,), (w_,))
            else:
                assert g.tobytes() == bytes([SENT]) * g.nbytes, (what, k)

    # patch family: dxy and status only
    full = ctx.orb_patch_search(0, I["xyl"], I["ref"], 3, **SEARCH)
    o = blank(full)
    assert lib.vido_orb_patch_search(ctx.h, 0, P(I["xyl"]), 3, 1, P(I["ref"]), 3, SEARCH["excl"], SEARCH["min_var"], SEARCH["min_zncc_q10"], SEARCH["peak_ratio_q10"],
                                     P(o[0]), None, None, P(o[3]), None, 0) == 0
    check("orb_patch_search", full, o, {0, 3})
    # Hamming family: no counters (the kernels count into the slot all the same)
    qd, qxy, ql, td, txy, tl = I["ham"]
    full = ctx.hamming_match_window(*I["ham"], **HAM)
    o = blank(full)
    assert lib.vido_hamming_match_window(ctx.h, P(qd), P(qxy), P(ql), 5, P(td), P(txy), P(tl), 70, HAM["radius"], HAM["level_tol"], HAM["max_dist"], 4, 5, 1,
                                         P(o[0]), P(o[1]), P(o[2]), P(o[3]), None, 0) == 0
    check("hamming_match_window", full, o, {0, 1, 2, 3})
    # flow family: the pair op with the marked flow and the status only (both q8 fields and the counters keep their slots), then the check with the status only
    a, b = I["pair"]
    full = ctx.dis_flow_pair(a, b, coarsest=2)
    o = blank(full)
    assert lib.vido_dis_flow_pair(ctx.h, P(a), P(b), 1, 0, 96, 96, 80, 2, 6, 1024, 0, 10, 32768, P(o[0]), None, None, P(o[3]), None, 0) == 0
    check("dis_flow_pair", full, o, {0, 3})
    fwd, bwd = I["check"]
    full = ctx.flow_consistency(fwd, bwd)
    o = blank(full)
    assert lib.vido_flow_consistency(ctx.h, P(fwd), P(bwd), 32, 40, 10, 32768, P(o[0]), None, None, 0) == 0
    check("flow_consistency", full, o, {0})
    # stereo family: q4 and the counters of the matcher; the filter's status alone, written over its input
    left, right = I["sgm"]
    full = ctx.stereo_sgm(left, right, max_disp=16)
    o = blank(full)
    assert lib.vido_stereo_sgm(ctx.h, P(left), P(right), 1, 0, 16, 16, 16, 16, 10, 120, 10, 1, None, P(o[1]), None, P(o[3]), 0) == 0
    check("stereo_sgm", full, o, {1, 3})
    q4, status = I["filt"]
    full = ctx.stereo_filter(q4, status, max_diff_q4=8, min_region=6)
    o = blank([full[0], full[1], full[0], full[3]])
    st = status.copy()
    assert lib.vido_stereo_filter(ctx.h, P(q4), P(st), 24, 16, 8, 6, C.c_float(0.0), None, P(st), None, None, 0) == 0
    _same("stereo_filter in place", (st,), (full[1],))
    check("stereo_filter", full, o, set())
