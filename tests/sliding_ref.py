"""Host restatement of sliding-window evaluation (ssseg/sliding.py, csrc/sliding.hip) in torch on the CPU, fp64 by
default: from the recorded per-window model outputs and the window rows to the fused map and the weight map.  It is
written window by window, as a scatter of whole crops with tensor ops -- the device code is a gather over accumulator
pixels -- and shares nothing with it but the definition in include/ssseg.h.  `dtype=torch.float32` runs the same
procedure in fp32: its deviation from the fp64 run is the yardstick of the GPU tests."""
import math

import torch
import torch.nn.functional as F

MIRROR, NULL = 1, 2


def plan(H, W, crop, stride):
    """window origins, row-major; the last window of an axis is moved back into the frame max(size, crop)"""
    def axis(size, c, s):
        frame = max(size, c)
        n = math.ceil((frame - c) / s) + 1
        return [min(i * s, frame - c) for i in range(n)]
    return [(y, x) for y in axis(H, crop[0], stride[0]) for x in axis(W, crop[1], stride[1])]


def rows(B, H, W, crop, stride, flip=False, window_batch=1):
    """the padded window list of one scale: (b, y0, x0, flags)"""
    r = [(b, y, x, 0) for b in range(B) for y, x in plan(H, W, crop, stride)]
    if flip:
        r = r + [(b, y, x, MIRROR) for b, y, x, _ in r]
    return r + [(0, 0, 0, NULL)] * (-len(r) % window_batch)


def scaled_size(H, W, s):
    return (H, W) if s == 1.0 else (int(H * s + 0.5), int(W * s + 0.5))


def resize(x, size):
    if tuple(x.shape[-2:]) == tuple(size):
        return x
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False)


def window_weight(crop, weighting, dtype):
    ch, cw = crop
    if weighting == 'uniform':
        return torch.ones(ch, cw, dtype=dtype)
    dy = torch.arange(ch, dtype=dtype) - (ch - 1) / 2
    dx = torch.arange(cw, dtype=dtype) - (cw - 1) / 2
    sy, sx = ch / 8, cw / 8
    return torch.exp(-((dy * dy / (2 * sy * sy))[:, None] + (dx * dx / (2 * sx * sx))[None, :]))


def activate(v, activation):
    if activation == 'softmax':
        return torch.softmax(v, dim=0)
    if activation == 'sigmoid':
        return torch.sigmoid(v)
    assert activation == 'none'
    return v


def fuse(outputs, table, B, frame, crop, activation='softmax', weighting='uniform', dtype=torch.float64):
    """outputs[j]: the model's [C,h,w] logits of window j of `table` (rows (b, y0, x0, flags), null rows included and
    ignored).  Returns (acc [B,C,Ha,Wa], wsum [B,Ha,Wa]): the weighted sums and the summed weights over `frame`."""
    ch, cw = crop
    C = outputs[0].shape[0]
    acc = torch.zeros(B, C, *frame, dtype=dtype)
    wsum = torch.zeros(B, *frame, dtype=dtype)
    wgt = window_weight(crop, weighting, dtype)
    for o, (b, y0, x0, flags) in zip(outputs, table):
        if flags & NULL:
            continue
        v = resize(o.to(dtype)[None], crop)[0]
        if flags & MIRROR:
            v = v.flip(-1)
        acc[b, :, y0:y0 + ch, x0:x0 + cw] += activate(v, activation) * wgt
        wsum[b, y0:y0 + ch, x0:x0 + cw] += wgt
    return acc, wsum


def merge(acc, wsum, interior, size):
    """the normalised map over the `interior` (Hs, Ws) of the frame, resized to `size`"""
    return resize((acc / wsum[:, None])[:, :, :interior[0], :interior[1]], size)


def fused_map(per_scale, B, size, crop, activation='softmax', weighting='uniform', dtype=torch.float64):
    """per_scale: one (outputs, table, (Hs, Ws)) triple per scale.  Returns the mean over the scales of the merged
    maps at `size`, and the weight map of the last scale."""
    total = None
    for outputs, table, (Hs, Ws) in per_scale:
        frame = (max(Hs, crop[0]), max(Ws, crop[1]))
        acc, wsum = fuse(outputs, table, B, frame, crop, activation, weighting, dtype)
        m = merge(acc, wsum, (Hs, Ws), size) * (1.0 / len(per_scale))
        total = m if total is None else total + m
    return total, wsum


# ---- stubs shared by the host and the GPU tests ------------------------------------------------------------------
def mix_weights(C, cin=3, seed=0):
    """integer mixing weights [C, cin] in [-3, 3], all rows distinct and non-zero"""
    g = torch.Generator().manual_seed(seed)
    while True:
        w = torch.randint(-3, 4, (C, cin), generator=g)
        if len({tuple(r) for r in w.tolist()}) == C and bool((w != 0).any(1).all()):
            return w.double()


def pointwise(image, w):
    """the whole-image function of the pointwise stub: logits[c] = sum_k w[c, k] image[k], per pixel"""
    return torch.einsum('ck,bkhw->bchw', w.to(image.dtype), image)


def integer_image(B, H, W, seed=0):
    """integer-valued channels in [1, 16): every mix (|.| <= 135), and every sum of up to 2^16 of them, is an exact fp32
    integer"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 16, (B, 3, H, W), generator=g).double()


def tiefree_image(B, H, W, seed=0):
    """channel k in +-{16^k, 2 * 16^k}: no integer combination with coefficients in [-6, 6], not all zero, vanishes
    (|d0 i0| <= 12 < 16 <= |d1 i1|, |d0 i0 + d1 i1| <= 204 < 256 <= |d2 i2|), so two distinct rows of mix_weights never
    tie at a pixel; the signs make the winning class vary from pixel to pixel; the mixes stay below 2^11"""
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([1., 16., 256.], dtype=torch.float64).view(1, 3, 1, 1)
    sign = torch.randint(0, 2, (B, 3, H, W), generator=g).double() * 2 - 1
    return base * sign * torch.randint(1, 3, (B, 3, H, W), generator=g).double()
