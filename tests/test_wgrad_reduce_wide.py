"""The many-split slab reduction of the weight gradient (wgrad_reduce_wide_kernel, conv_wgrad.hip), exact, in both of
its load widths.

Operands are the small integers of tests/exact.py: every product and every partial sum is an exact integer far below
2^24 whatever the order of the additions, so dW must EQUAL the fp64 CPU result -- in both output layouts, with and
without accumulate, with real channel counts that cut a 16-byte piece, and where the weight count is no multiple of
the block's 256 outputs.  That the kernel keeps its ORDER of additions (which matters only on inexact data) is what the
benchmark's --dump-outputs comparison against the parent shows.
"""
import ctypes

import pytest
import torch

import exact

pytestmark = pytest.mark.gpu

H = W = 200   # one image: 40000 pixels, 70 splits of 576 pixels for the geometries below

# (C, K, k, c_real, k_real).  The launch takes 16-byte loads (a block owns 256 outputs) from 32768 weights on and the
# 4-byte form (64 outputs) below that; the sums and their order are the same.
#   4-byte:  1x1 64 -> 64 (4096 weights); 1x1 24 -> 40 with 22 / 37 real (960 weights: a ragged last block); 3x3 16 -> 8
#            (1152 weights, taps)
#   16-byte: 3x3 64 -> 64 (36864 weights = 144 blocks, taps); 1x1 136 -> 248 with 134 / 245 real (33728 weights: 131.75
#            blocks, and the real channels end inside a 16-byte piece)
GEOMS = [(64, 64, 1, 64, 64), (24, 40, 1, 22, 37), (16, 8, 3, 16, 8), (64, 64, 3, 64, 64), (136, 248, 1, 134, 245)]


@pytest.fixture(scope='module')
def lib():
    from ssseg import native as N
    return N


def _operands(C, K, k):
    g = exact._gen('wide-reduce', C, K, k)
    x = exact.ints((1, C, H, W), -2, 2, 0.75, g)
    gy = exact.ints((1, K, H, W), -2, 2, 0.75, g)
    xp = torch.nn.functional.pad(x, (k // 2,) * 4)
    cols = torch.nn.functional.unfold(xp, k)                       # [1, C k k, H W]
    dw = (gy.reshape(K, H * W) @ cols[0].t()).reshape(K, C, k, k)  # fp64: exact integers
    assert float(dw.abs().max()) < 2 ** 24 and int((dw != 0).sum()) > dw.numel() // 2
    return x, gy, dw


@pytest.mark.parametrize('C,K,k,c_real,k_real', GEOMS, ids=lambda v: str(v))
def test_wide_reduce_exact(hip_device, lib, C, K, k, c_real, k_real):
    N = lib
    x, gy, dw = _operands(C, K, k)
    xd = x.permute(0, 2, 3, 1).contiguous().to(hip_device, torch.bfloat16)
    gd = gy.permute(0, 2, 3, 1).contiguous().to(hip_device, torch.bfloat16)
    d = N.ConvDesc()
    for name, v in dict(N=1, H=H, W=W, C=C, ldx=C, OH=H, OW=W, K=K, R=k, S=k, sy=1, sx=1, dy=1, dx=1, py=-(k // 2),
                        px=-(k // 2), outH=H, outW=W, osy=1, osx=1, ooy=0, oox=0, ldy=K, ldw=k * k * C).items():
        setattr(d, name, v)
    nb = N.lib().ssseg_conv_wgrad_workspace_bytes(ctypes.byref(d), N.BF16)
    splits = (nb - 256) // (K * k * k * C * 4)
    assert splits >= 64, f'the plan gives {splits} splits: the wide reduction is not the kernel under test'
    ws = torch.empty(nb, dtype=torch.uint8, device=hip_device)
    base_g = exact._gen('wide-reduce-base', C, K, k)
    for layout in (0, 1):
        shape = (K, k, k, C) if layout == 0 else (k_real, c_real, k, k)
        base = exact.ints(shape, -8, 8, 1.0, base_g).float()
        want_sum = dw[:k_real, :c_real]
        for accumulate in (0, 1):
            out = base.clone().to(hip_device)
            N.call('ssseg_conv_wgrad', N.dev_ptr(xd), N.dev_ptr(gd), N.dev_ptr(out), ctypes.byref(d), N.BF16, c_real,
                   k_real, layout, accumulate, N.dev_ptr(ws), nb, N.stream())
            want = base.double().clone()
            if layout == 0:
                real = want[:k_real, :, :, :c_real]
                real.copy_(want_sum.permute(0, 2, 3, 1) + (real if accumulate else 0))
            else:
                want.copy_(want_sum + (want if accumulate else 0))
            assert torch.equal(out.cpu().double(), want), (layout, accumulate)
