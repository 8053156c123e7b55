"""CPU: pack_gconv3x3_h (vido_slam_amd/nets/ops.py), the weight side of the split-fp16 grouped 3x3 kernel (csrc/gconvh.hip): the two fp16 planes times the inverse
channel scales give the weight back to 2^-22 relative, every element sits where the kernel's A operand reads it, and shapes the kernel does not take give None."""
import pytest
import torch

from vido_slam_amd.nets.ops import pack_gconv3x3_h


def _weight(groups, cpg, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(groups * cpg, cpg, 3, 3, generator=g) * torch.exp(2 * torch.randn(groups * cpg, 1, 1, 1, generator=g))      # heavy-tailed channel scales
    w[1] = 0.0                                                                                                                     # a folded batch norm with gamma = 0
    return w


@pytest.mark.parametrize("groups,cpg", [(3, 32), (2, 64)])
def test_planes_times_scales_reproduce_the_weight(groups, cpg):
    w = _weight(groups, cpg, 11 * groups + cpg)
    p = pack_gconv3x3_h(w, groups)
    cout = groups * cpg
    assert p.dtype == torch.int16 and p.numel() == 2 * cout * (cpg * 9 + 1)
    n = 2 * cout * cpg * 9
    inv = p[n:].view(torch.float32).double()
    assert inv.numel() == cout and bool((torch.frexp(inv.float())[0] == 0.5).all()), "inverse scales are powers of two"
    # [g][cob][step][tap][plane][k half][co32][k8] -> [plane][co][ci][tap]
    planes = p[:n].view(torch.float16).double().reshape(groups, cpg // 32, cpg // 16, 9, 2, 2, 32, 8)
    planes = planes.permute(4, 0, 1, 6, 2, 5, 7, 3).reshape(2, cout, cpg, 9)
    back = (planes[0] + planes[1] / 2048.0) * inv[:, None, None]
    wd = w.double().reshape(cout, cpg, 9)
    # 2^-22 of the element, down to 2^-26 of the channel's largest weight (below that the absolute floor of split_f16x2)
    tol = 2.0 ** -22 * wd.abs() + 2.0 ** -48 * wd.abs().amax((1, 2), keepdim=True)
    assert bool(((back - wd).abs() <= tol).all()), float(((back - wd).abs() / tol.clamp_min(1e-300)).max())
    assert bool((back[1] == 0).all())
    # the largest |w| of a channel sits in [2^14, 2^15) of its scale
    top = (wd.abs().amax((1, 2)) / inv)
    nz = top > 0
    assert bool(((top[nz] >= 2.0 ** 14) & (top[nz] < 2.0 ** 15)).all())


def test_unsupported_shapes_give_none():
    assert pack_gconv3x3_h(torch.zeros(32, 16, 3, 3), 2) is None            # 16 channels per group
    assert pack_gconv3x3_h(torch.zeros(256, 128, 3, 3), 2) is None          # 128 channels per group
    assert pack_gconv3x3_h(torch.zeros(64, 32, 1, 1), 2) is None            # not 3 x 3
    assert pack_gconv3x3_h(torch.zeros(64, 32, 3, 3), 1) is None            # 64 outputs from 32 inputs in one group
    assert pack_gconv3x3_h(torch.zeros(64, 32, 3, 3), 2) is not None
