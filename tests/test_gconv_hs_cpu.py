"""CPU: the host side of the split-fp16 grouped 3x3 kernel for 8 / 16 channels per group (csrc/gconvhs.hip).

pack_gconv3x3_hs (vido_slam_amd/nets/ops.py): the two fp16 planes times the inverse channel scales give the weight back to 2^-22 relative, every element sits where the kernel's A
operand reads it (lane 16 b + row of instruction i holds the 8 input channels of block b's (tap, channel group) slot), zero slots and zero rows are zero, and shapes the kernel
does not take give None.

The plan (vido_debug_ghs_plan) walked on the CPU as the kernel walks it: per chunk a ring of RING slots addressed by (padded flat position) & (RING - 1), the first round's band
filled in load steps, every later round's RL new positions stored after the round that still needs the slots they replace.  Every tap of every output must find the element the
convolution's definition names (or the zero of an out-of-range offset for padding), every output is produced once, every chunk starts inside the image, and the elements loaded
per channel — counted by the walk, equal to what the host computes from the plan — do not exceed what the plan of the fp32 kernel k_gconv3x3_m16d (vido_debug_gc16_plan) loads at
the same shape (where that kernel has no plan, W % 4 != 0 here, the shapes are single items and every element is loaded exactly once)."""
import ctypes as C

import numpy as np
import pytest
import torch

from vido_slam_amd.nets.ops import pack_gconv3x3_hs


def _weight(groups, cpg, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(groups * cpg, cpg, 3, 3, generator=g) * torch.exp(2 * torch.randn(groups * cpg, 1, 1, 1, generator=g))      # heavy-tailed channel scales
    w[1] = 0.0                                                                                                                     # a folded batch norm with gamma = 0
    return w


def _slot(cpg, i, b):
    """(tap, channel group) of block b of instruction i, as csrc/gconvhs.hip assigns them"""
    return (4 * i + b, 0) if cpg == 8 else (2 * i + (b >> 1), b & 1)


@pytest.mark.parametrize("groups,cpg", [(3, 8), (2, 16)])
def test_planes_times_scales_reproduce_the_weight(groups, cpg):
    w = _weight(groups, cpg, 11 * groups + cpg)
    p = pack_gconv3x3_hs(w, groups)
    cout = groups * cpg; ni = 3 if cpg == 8 else 5
    n = groups * ni * 1024
    assert p.dtype == torch.int16 and p.numel() == n + 2 * cout
    inv = p[n:].view(torch.float32).double()
    assert inv.numel() == cout and bool((torch.frexp(inv.float())[0] == 0.5).all()), "inverse scales are powers of two"
    planes = p[:n].view(torch.float16).double().reshape(groups, ni, 2, 4, 16, 8)      # [g][instruction][plane][block][row][k8]: lane 16 block + row reads 8 fp16
    back = torch.zeros(2, cout, cpg, 9, dtype=torch.float64)
    seen = torch.zeros(cpg, 9, dtype=torch.int64)
    for i in range(ni):
        for b in range(4):
            tap, cg = _slot(cpg, i, b)
            blk = planes[:, i, :, b]                                                    # [g][plane][row][k8]
            assert bool((blk[:, :, cpg:] == 0).all()), "rows past the group's output channels are zero"
            if tap >= 9:
                assert bool((blk == 0).all()), "a zero slot is zero"
                continue
            back[:, :, 8 * cg:8 * cg + 8, tap] = blk[:, :, :cpg].permute(1, 0, 2, 3).reshape(2, cout, 8)
            seen[8 * cg:8 * cg + 8, tap] += 1
    assert bool((seen == 1).all()), "every (input channel, tap) has exactly one slot"
    got = (back[0] + back[1] / 2048.0) * inv[:, None, None]
    wd = w.double().reshape(cout, cpg, 9)
    # 2^-22 of the element, down to 2^-26 of the channel's largest weight (below that the absolute floor of split_f16x2)
    tol = 2.0 ** -22 * wd.abs() + 2.0 ** -48 * wd.abs().amax((1, 2), keepdim=True)
    assert bool(((got - wd).abs() <= tol).all()), float(((got - wd).abs() / tol.clamp_min(1e-300)).max())
    assert bool((got[1] == 0).all())
    top = (wd.abs().amax((1, 2)) / inv)                                                 # the largest |w| of a channel sits in [2^14, 2^15) of its scale
    nz = top > 0
    assert bool(((top[nz] >= 2.0 ** 14) & (top[nz] < 2.0 ** 15)).all())


def test_unsupported_shapes_give_none():
    assert pack_gconv3x3_hs(torch.zeros(64, 32, 3, 3), 2) is None            # 32 channels per group
    assert pack_gconv3x3_hs(torch.zeros(128, 64, 3, 3), 2) is None           # 64
    assert pack_gconv3x3_hs(torch.zeros(8, 4, 3, 3), 2) is None              # 4
    assert pack_gconv3x3_hs(torch.zeros(16, 8, 1, 1), 2) is None             # not 3 x 3
    assert pack_gconv3x3_hs(torch.zeros(16, 8, 5, 5), 2) is None
    assert pack_gconv3x3_hs(torch.zeros(16, 8, 3, 3), 1) is None             # 16 outputs from 8 inputs in one group
    assert pack_gconv3x3_hs(torch.zeros(32, 8, 3, 3), 2) is None             # 8 -> 16 per group
    assert pack_gconv3x3_hs(torch.zeros(16, 8, 3, 3), 2) is not None and pack_gconv3x3_hs(torch.zeros(32, 16, 3, 3), 2) is not None


def _lib():
    from vido_slam_amd.host import load_library
    lib = load_library()
    lib.vido_debug_ghs_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    lib.vido_debug_ghs_plan.restype = C.c_int
    return lib


def _fp32_loaded(lib, H, W, cpg):
    """elements per channel that k_gconv3x3_m16d's plan loads: R rows from row r0 - 1 on per chunk, those inside the image; None where that kernel has no plan"""
    out = (C.c_int * 6)()
    if lib.vido_debug_gc16_plan(H, W, 8, cpg, out) != 1:
        return None
    R, _, _, gx, P, Wpd = list(out)
    n = 0
    for chunk in range(gx):
        r0 = chunk * P // Wpd
        n += max(0, min(H, r0 - 1 + R) - max(0, r0 - 1)) * W
    return n


WALK = ((3, 4, 8), (7, 9, 8), (17, 20, 8), (3, 140, 8), (200, 272, 8), (100, 136, 16), (272, 200, 8), (136, 100, 16), (5, 33, 16))


@pytest.mark.parametrize("H,W,cpg", WALK, ids=lambda v: str(v))
def test_ring_walk_resolves_every_tap_and_loads_no_more_than_the_fp32_plan(H, W, cpg):
    lib = _lib()
    out = (C.c_int * 7)(); loaded = C.c_longlong(0)
    assert lib.vido_debug_ghs_plan(32, H, W, cpg, cpg, out, C.byref(loaded)) == 1
    gx, CL, RL, RING, Wp, STEP, NI = list(out)
    npos, halo, RM = H * Wp, 2 * Wp + 2, RING - 1
    assert Wp == W + 2 and NI == (3 if cpg == 8 else 5) and STEP == 256 * 4 // (cpg // 8)
    assert RING & RM == 0 and RL % 64 == 0 and 64 <= RL <= STEP and RL + halo <= RING and CL % 16 == 0 and gx == -(-npos // CL)
    assert RING * 32 * (cpg // 8) <= 64 * 1024, "two workgroups per CU at the least"
    if gx > 1:
        assert CL >= max(512, 3 * halo), "an item re-reads at most a third of what it computes"
    done = np.zeros((H, W), dtype=np.int64)
    nload = 0
    for chunk in range(gx):
        qc = chunk * CL
        assert qc < npos, "every item starts inside the image"
        qn = min(CL, npos - qc); pend = qc + qn + halo; nrounds = -(-qn // RL)
        ring = np.full(RING, -2, dtype=np.int64)                                        # element index y W + x a slot holds; -1: the zero of an out-of-range offset; -2: never written

        def load(p0, n):
            if n <= 0:
                return 0
            assert n <= STEP
            f = p0 + np.arange(n); yr, xc = f // Wp, f % Wp
            ok = (f < pend) & (yr >= 1) & (yr <= H) & (xc >= 1) & (xc <= W)
            ring[f & RM] = np.where(ok, (yr - 1) * W + (xc - 1), -1)
            return int(ok.sum())

        n0 = min(RL + halo, pend - qc)
        for s in range(0, n0, STEP):
            nload += load(qc + s, min(STEP, n0 - s))
        for rd in range(nrounds):
            q0 = qc + rd * RL
            q = np.arange(q0, min(q0 + RL, qc + qn)); yy, xx = q // Wp, q % Wp
            keep = xx < W; q, yy, xx = q[keep], yy[keep], xx[keep]
            for dy in range(3):
                for dx in range(3):
                    yi, xi = yy + dy - 1, xx + dx - 1
                    want = np.where((yi >= 0) & (yi < H) & (xi >= 0) & (xi < W), yi * W + xi, -1)
                    got = ring[(q + dy * Wp + dx) & RM]
                    assert np.array_equal(got, want), (H, W, cpg, chunk, rd, dy, dx)
            assert (ring[q & RM] != -2).all(), "a zero slot (tap 0's address) reads written data"
            np.add.at(done, (yy, xx), 1)
            if rd + 1 < nrounds:                                                        # the new positions, stored once the round is over
                pn = q0 + RL + halo
                nload += load(pn, min(RL, pend - pn))
    assert (done == 1).all(), "every output is produced exactly once"
    assert nload == loaded.value, "the host's count of loaded elements is the walk's"
    ref = _fp32_loaded(lib, H, W, cpg)
    print("gconv3x3_hs plan %dx%d cpg %d: gx %d CL %d RL %d RING %d; loaded per channel %d = %.3f x the image; fp32 plan %s" % (H, W, cpg, gx, CL, RL, RING, nload, nload / (H * W), ref))
    if ref is None:
        assert gx == 1 and nload == H * W
    else:
        assert nload <= ref, (nload, ref)
    assert nload <= 1.5 * H * W


def test_load_units_of_16_per_group_cover_a_step_once():
    """the kernel's unit -> (position, channel group) map at 16 per group: the halves of a wave take the two channel groups of 32 consecutive positions"""
    u = np.arange(1024)
    pos, cg = ((u >> 6) << 5) | (u & 31), (u >> 5) & 1
    assert sorted(zip(pos.tolist(), cg.tolist())) == [(p, c) for p in range(512) for c in range(2)]


def test_supported_and_plan_limits():
    lib = _lib()
    s = lib.vido_gconv3x3_hs_supported
    assert s(200, 272, 8, 8) and s(100, 136, 16, 16) and s(1, 1, 8, 8) and s(7, 9, 16, 16) and s(5, 957, 8, 8) and s(5, 445, 16, 16)
    assert not s(5, 958, 8, 8) and not s(5, 446, 16, 16)                    # the ring of a round no longer fits half a CU's LDS
    assert not s(50, 68, 32, 32) and not s(50, 68, 8, 16) and not s(50, 68, 4, 4) and not s(0, 68, 8, 8) and not s(50, 0, 16, 16)
    assert lib.vido_gconv3x3_h_supported(50, 68, 16, 16) == 0               # the 32 / 64 kernel keeps declining these
    assert lib.vido_debug_ghs_plan(32, 50, 68, 32, 32, (C.c_int * 7)(), None) == 0
