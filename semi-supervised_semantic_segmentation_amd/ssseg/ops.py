"""Autograd-aware wrappers over libssseg.so for the loss / CowMix / EMA part of the hot path.

Each function documents the reference call site it replaces.  Inputs must be HIP tensors.
"""
import ctypes
import os

import torch

from . import native as N


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# CowMix (cowmix.py)
# ------------------------------------------------------------------------------------------------
def cowmix_mask(noise, sigma, p, return_field=False):
    """Mask arithmetic of generate_cowmix_masks_like (cowmix.py:40-69).

    noise [B,1,H,W] or [B,H,W] f32, sigma [B], p [B] (device tensors) -> mask [B,1,H,W] f32.
    """
    B = noise.shape[0]
    H, W = noise.shape[-2:]
    noise = _c(noise.float())
    sigma = _c(sigma.float().to(noise.device))
    p = _c(p.float().to(noise.device))
    mask = torch.empty(B, 1, H, W, device=noise.device, dtype=torch.float32)
    field = torch.empty_like(mask) if return_field else None
    thr = torch.empty(B, device=noise.device, dtype=torch.float32) if return_field else None
    nb = N.lib().ssseg_cowmix_workspace_bytes(B, H, W)
    ws = N.workspace(nb, noise.device)
    N.call('ssseg_cowmix_mask', N.dev_ptr(noise, 'noise'), N.dev_ptr(sigma), N.dev_ptr(p), B, H, W, N.dev_ptr(mask),
           N.dev_ptr(field) if field is not None else None, N.dev_ptr(thr) if thr is not None else None,
           N.dev_ptr(ws), nb, N.stream())
    if return_field:
        return mask, field, thr
    return mask


def normal_(out, seed, offset):
    N.call('ssseg_normal_f32', N.dev_ptr(out, 'out'), out.numel(), int(seed) & (2 ** 64 - 1),
           int(offset) & (2 ** 64 - 1), N.stream())
    return out


def mix(a, b, mask):
    """mix_with_mask (cowmix.py:72-73): a*m + b*(1-m), mask [B,1,H,W] broadcast over channels."""
    a, b = _c(a), _c(b)
    m = _c(mask.float())
    out = torch.empty_like(a)
    B, C = a.shape[0], a.shape[1]
    HW = a[0, 0].numel()
    N.call('ssseg_mix', N.dev_ptr(a, 'a'), N.dev_ptr(b, 'b'), N.dev_ptr(m, 'mask'), N.dev_ptr(out), B, C, HW,
           N.dt_code(a), N.stream())
    return out


def classmix_mask(teacher_logits, keys, return_state=False):
    """ClassMix mask (Olsson et al. 2021) of the teacher's logits [B,C,H,W] (fp32, bf16 or fp16; 1 <= C <= 64): the
    label of a pixel is its argmax (first maximum wins, NaN counts as the maximum); per image, of the n classes
    present, the ceil(n/2) with the smallest (keys[b,c], c) are chosen; mask [B,1,H,W] f32 is 1 on their pixels.
    keys [B,C] integers in [0, 2^31).  return_state: also (present, chosen) [B] int64, bit c = class c."""
    x = teacher_logits
    if x.dim() != 4:
        raise ValueError(f'classmix_mask: logits must be [B,C,H,W], got {tuple(x.shape)}')
    B, C, H, W = x.shape
    if not 1 <= C <= 64:
        raise ValueError(f'classmix_mask: {C} channels (1 to 64 are supported)')
    if tuple(keys.shape) != (B, C):
        raise ValueError(f'classmix_mask: keys must be [B,C] = {(B, C)}, got {tuple(keys.shape)}')
    with torch.no_grad():
        x = x.detach()
        if x.stride(2) != W * x.stride(3) and H != 1:
            x = x.contiguous()   # the kernel walks the pixels of an image at one stride (NCHW and channels-last do)
        keys = _c(keys.to(torch.int32))
        mask = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32)
        present = torch.empty(B, device=x.device, dtype=torch.int64) if return_state else None
        chosen = torch.empty(B, device=x.device, dtype=torch.int64) if return_state else None
        nb = N.lib().ssseg_classmix_workspace_bytes(B, H, W)
        ws = N.workspace(nb, x.device)
        N.call('ssseg_classmix_mask', N.dev_ptr(x, 'logits'), N.strides4(x), N.dt_code(x), N.dev_ptr(keys, 'keys'), B,
               C, H, W, N.dev_ptr(mask), N.dev_ptr(present), N.dev_ptr(chosen), N.dev_ptr(ws), nb, N.stream())
    return (mask, present, chosen) if return_state else mask


def cutmix_mask(params, H, W, mask_proportion_range, return_boxes=False):
    """CutMix mask (French et al. 2020): params [B,4] uniforms (p', u, v1, v2) in [0,1) -> mask [B,1,H,W] f32, 1 inside
    the box  p = lo + (hi-lo) p', h = rint(H p^u), w = rint(W p^(1-u)), top = rint((H-h) v1), left = rint((W-w) v2)
    (fp64, half to even).  return_boxes: also [B,4] int32 (top, left, h, w)."""
    if params.dim() != 2 or params.shape[1] != 4:
        raise ValueError(f'cutmix_mask: params must be [B,4], got {tuple(params.shape)}')
    lo, hi = float(mask_proportion_range[0]), float(mask_proportion_range[1])
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f'cutmix_mask: mask_proportion_range {mask_proportion_range!r} is not 0 <= lo <= hi <= 1')
    with torch.no_grad():
        params = _c(params.detach().float())
        B = params.shape[0]
        mask = torch.empty(B, 1, H, W, device=params.device, dtype=torch.float32)
        boxes = torch.empty(B, 4, device=params.device, dtype=torch.int32) if return_boxes else None
        N.call('ssseg_cutmix_mask', N.dev_ptr(params, 'params'), B, H, W, lo, hi, N.dev_ptr(mask), N.dev_ptr(boxes),
               N.stream())
    return (mask, boxes) if return_boxes else mask


# ------------------------------------------------------------------------------------------------
# Bilinear interpolation (F.interpolate mode='bilinear')
# ------------------------------------------------------------------------------------------------
def _axpby(x, a, y=None, b=0.0):
    out = torch.empty_like(x)
    N.call('ssseg_axpby', N.dev_ptr(x), float(a), N.dev_ptr(y) if y is not None else None, float(b), N.dev_ptr(out),
           x.numel(), N.stream())
    return out


class _Axpby(torch.autograd.Function):
    """a*x (+ b*y): the loss-term arithmetic on the device (no framework elementwise kernels)"""
    @staticmethod
    def forward(ctx, x, a, y, b):
        ctx.a, ctx.b, ctx.has_y = a, b, y is not None
        return _axpby(_c(x), a, _c(y) if y is not None else None, b)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        gx = _axpby(g, ctx.a) if ctx.a != 1.0 else g
        gy = None
        if ctx.has_y:
            gy = _axpby(g, ctx.b) if ctx.b != 1.0 else g
        return gx, None, gy, None


def scale(x, a):
    """a * x for a device loss tensor (autograd)."""
    return _Axpby.apply(x, float(a), None, 0.0)


def add_scaled(x, y, b=1.0):
    """x + b * y for device loss tensors (autograd)."""
    return _Axpby.apply(x, 1.0, y, float(b))


_ONES = {}


def backward(loss):
    """loss.backward() seeded from a cached device 1.0 (autograd's own seed is a framework fill kernel)."""
    key = (loss.device, loss.dtype, tuple(loss.shape))
    one = _ONES.get(key)
    if one is None:
        one = torch.ones_like(loss)
        _ONES[key] = one
    loss.backward(one)


class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, align_corners):
        Nn, C, H, W = x.shape
        Ho, Wo = int(size[0]), int(size[1])
        fmt = torch.channels_last if (x.is_contiguous(memory_format=torch.channels_last) and C > 1
                                      and not x.is_contiguous()) else torch.contiguous_format
        y = torch.empty((Nn, C, Ho, Wo), device=x.device, dtype=x.dtype, memory_format=fmt)
        N.call('ssseg_bilinear_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(y), Nn, C, H, W, Ho, Wo, N.strides4(x),
               N.strides4(y), int(bool(align_corners)), N.dt_code(x), N.stream())
        ctx.meta = (Nn, C, H, W, Ho, Wo, bool(align_corners), fmt)
        return y

    @staticmethod
    def backward(ctx, gy):
        Nn, C, H, W, Ho, Wo, ac, fmt = ctx.meta
        gx = torch.empty((Nn, C, H, W), device=gy.device, dtype=gy.dtype, memory_format=fmt)
        N.call('ssseg_bilinear_bwd', N.dev_ptr(gy, 'gy'), N.dev_ptr(gx), Nn, C, H, W, Ho, Wo, N.strides4(gy),
               N.strides4(gx), int(ac), N.dt_code(gy), N.stream())
        return gx, None, None


_IDENTITY_RESIZE = os.environ.get('SSSEG_BILINEAR_IDENTITY', '1') != '0'   # (A/B switch: 0 = always launch)


def interpolate_bilinear(x, size, align_corners=False):
    """F.interpolate(x, size, mode='bilinear', align_corners=...) on the device.  At the input's own size the sampling
    weights are (1, 0) for either align_corners -- the values are the input's -- and PyTorch's CPU kernels copy the
    input there ('special case: just copy'), so x itself is returned (the logits-to-mask-size resizes of the training
    step, train.py:71,74,93 and losses.py:18, are all identity-sized on the benchmark geometry) when it is dense NCHW
    or channels_last; the kernel would write the same layout."""
    size = (int(size[0]), int(size[1]))
    if _IDENTITY_RESIZE and x.dim() == 4 and tuple(x.shape[2:4]) == size and (
            x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        return x
    return _Bilinear.apply(x, size, align_corners)


class _Rotate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, angle):
        x = _c(x.float())
        y = torch.empty_like(x)
        Nn, C, H, W = x.shape
        N.call('ssseg_rotate_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(y), Nn, C, H, W, float(angle), N.stream())
        ctx.meta = (Nn, C, H, W, float(angle))
        return y

    @staticmethod
    def backward(ctx, gy):
        Nn, C, H, W, angle = ctx.meta
        gy = _c(gy.float())
        gx = torch.empty_like(gy)
        N.call('ssseg_rotate_bwd', N.dev_ptr(gy), N.dev_ptr(gx), Nn, C, H, W, angle, N.stream())
        return gx, None


def rotate(x, angle_deg):
    """kornia.rotate(x, angle) for NCHW fp32 (reversible_augmentations.py:13-23): counter-clockwise degrees
    about the image centre, bilinear, zero padding; differentiable."""
    return _Rotate.apply(x, angle_deg)


def affine_mats(angles_deg, scales, H, W, device):
    """Per-sample matrices of the affine warp (include/ssseg.h, ssseg_affine_warp_fwd): A(theta_b, s_b) and its
    inverse A(-theta_b, 1/s_b), [B, 6] fp32 each, built on the host in fp64, rounded once and uploaded."""
    th = torch.deg2rad(torch.as_tensor(angles_deg, dtype=torch.float64).reshape(-1).cpu())
    s = torch.as_tensor(scales, dtype=torch.float64).reshape(-1).cpu()
    if th.numel() != s.numel():
        raise ValueError('affine_mats: one angle and one scale per sample')
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0

    def mat(al, be):
        return torch.stack([al, be, cx - al * cx - be * cy, -be, al, cy + be * cx - al * cy], 1)
    mats = mat(torch.cos(th) / s, -torch.sin(th) / s)
    inv = mat(torch.cos(th) * s, torch.sin(th) * s)
    return mats.float().to(device), inv.float().to(device)


def _dense_like(x):
    """an empty tensor of x's shape and dtype: channels-last where x is, NCHW otherwise"""
    fmt = torch.channels_last if (x.is_contiguous(memory_format=torch.channels_last) and x.shape[1] > 1
                                  and not x.is_contiguous()) else torch.contiguous_format
    return torch.empty(tuple(x.shape), device=x.device, dtype=x.dtype, memory_format=fmt)


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mats, mats_inv, want_valid):
        Nn, C, H, W = x.shape
        if tuple(mats.shape) != (Nn, 6) or tuple(mats_inv.shape) != (Nn, 6):
            raise ValueError('affine_warp: mats and mats_inv must be [N, 6]')
        mats, mats_inv = _c(mats.float()), _c(mats_inv.float())
        y = _dense_like(x)
        valid = torch.empty((Nn, H, W), device=x.device, dtype=torch.float32) if want_valid else None
        N.call('ssseg_affine_warp_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(y), N.dev_ptr(mats, 'mats'), Nn, C, H, W,
               N.strides4(x), N.strides4(y), N.dt_code(x), N.dev_ptr(valid), N.stream())
        ctx.save_for_backward(mats, mats_inv)
        ctx.set_materialize_grads(False)   # no zero-filled gradient for the validity map
        if not want_valid:
            return y
        ctx.mark_non_differentiable(valid)
        return y, valid

    @staticmethod
    def backward(ctx, gy, g_valid=None):
        if gy is None:
            return None, None, None, None
        mats, mats_inv = ctx.saved_tensors
        Nn, C, H, W = gy.shape
        gx = _dense_like(gy)
        N.call('ssseg_affine_warp_bwd', N.dev_ptr(gy, 'gy'), N.dev_ptr(gx), N.dev_ptr(mats), N.dev_ptr(mats_inv), Nn, C,
               H, W, N.strides4(gy), N.strides4(gx), N.dt_code(gy), N.stream())
        return gx, None, None, None


def affine_warp(x, mats, mats_inv, want_valid=False):
    """y[n] = bilinear sample of x[n] at mats[n] applied to each output pixel (zeros outside), any of fp32 / bf16 /
    fp16, NCHW or channels-last; differentiable in x (the gather adjoint ssseg_affine_warp_bwd, which needs
    mats_inv).  want_valid: also the [N, H, W] fp32 map of the pixels whose sampling point lies in the image."""
    return _AffineWarp.apply(x, mats, mats_inv, bool(want_valid))


class _Sigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x.float())
        y = torch.empty_like(x)
        N.call('ssseg_sigmoid_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(y), x.numel(), N.stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = _c(gy.float())
        gx = torch.empty_like(y)
        N.call('ssseg_sigmoid_bwd', N.dev_ptr(y), N.dev_ptr(gy), N.dev_ptr(gx), y.numel(), N.stream())
        return gx


def sigmoid(x):
    """torch.sigmoid (fp32, any layout -> contiguous): the probability map the discriminator sees."""
    return _Sigmoid.apply(x)


# ------------------------------------------------------------------------------------------------
# Losses
# ------------------------------------------------------------------------------------------------
class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        x, t = _c(x.float()), _c(t.float())
        out = torch.empty((), device=x.device, dtype=torch.float32)
        nb = N.lib().ssseg_reduce_workspace_bytes(x.numel())
        ws = N.workspace(nb, x.device)
        N.call('ssseg_bce_logits_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(t, 'target'), x.numel(), N.dev_ptr(out),
               N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_bce_logits_bwd', N.dev_ptr(x), N.dev_ptr(t), x.numel(), N.dev_ptr(g), N.dev_ptr(gx), N.stream())
        return gx, None


def bce_with_logits_mean(x, t):
    """F.binary_cross_entropy_with_logits(x, t, reduction='mean') (losses.py:47)."""
    return _BCE.apply(x, t)


class _Consistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, thr, w):
        s, t = _c(s.float()), _c(t.float())
        B, C = s.shape[:2]
        HW = s[0, 0].numel()
        out = torch.empty(3, device=s.device, dtype=torch.float32)
        nb = N.lib().ssseg_reduce_workspace_bytes(B * HW)
        ws = N.workspace(nb, s.device)
        if w is None:
            N.call('ssseg_consistency_fwd', N.dev_ptr(s, 'student'), N.dev_ptr(t, 'teacher'), B, C, HW, float(thr),
                   N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
            ctx.save_for_backward(s, t, out)
        else:
            w = _c(w.float())
            if w.numel() != B * HW:
                raise ValueError('consistency_loss_weighted: w must hold one weight per pixel, [B, H, W]')
            N.call('ssseg_consistency_w_fwd', N.dev_ptr(s, 'student'), N.dev_ptr(t, 'teacher'), N.dev_ptr(w, 'w'), B, C,
                   HW, float(thr), N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
            ctx.save_for_backward(s, t, out, w)
        ctx.meta = (B, C, HW, float(thr))
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)   # no zero-filled gradient for the cm output (a framework fill kernel)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_loss, g_cm):
        s, t, out = ctx.saved_tensors[:3]
        B, C, HW, thr = ctx.meta
        gs = torch.empty_like(s)
        g = _c(g_loss.float())
        if len(ctx.saved_tensors) == 3:
            N.call('ssseg_consistency_bwd', N.dev_ptr(s), N.dev_ptr(t), B, C, HW, thr, N.dev_ptr(out), N.dev_ptr(g),
                   N.dev_ptr(gs), N.stream())
        else:
            N.call('ssseg_consistency_w_bwd', N.dev_ptr(s), N.dev_ptr(t), N.dev_ptr(ctx.saved_tensors[3]), B, C, HW,
                   thr, N.dev_ptr(out), N.dev_ptr(g), N.dev_ptr(gs), N.stream())
        return gs, None, None, None


def consistency_loss(student_logits, teacher_logits, thr):
    """train.py:97-108: returns (loss, confidence_modulator.mean()); loss is NaN when no pixel is confident."""
    return _Consistency.apply(student_logits, teacher_logits, thr, None)


def consistency_loss_weighted(student_logits, teacher_logits, w, thr):
    """consistency_loss with the confidence modulator multiplied by w [B, H, W] (the validity map of a warped-back
    student view): (sum d^2 cm w / sum cm w, sum cm w / npix); NaN when no weighted pixel is confident.  w is a
    constant (no gradient)."""
    return _Consistency.apply(student_logits, teacher_logits, thr, w)


def _device_checked(name, **tensors):
    for n, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise ValueError(f'{name}: {n} must be a HIP device tensor (no CPU fallback), got {t.device}')


class _ConsistencySoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, thr, w):
        s, t = _c(s.float()), _c(t.float())
        B, C = s.shape[:2]
        HW = s[0, 0].numel()
        out = torch.empty(3, device=s.device, dtype=torch.float32)
        nb = N.lib().ssseg_reduce_workspace_bytes(B * HW)
        ws = N.workspace(nb, s.device)
        if w is not None:
            w = _c(w.float())
        N.call('ssseg_consistency_sm_fwd', N.dev_ptr(s, 'student'), N.dev_ptr(t, 'teacher'), N.dev_ptr(w, 'w'), B, C,
               HW, float(thr), N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        if w is None:
            ctx.save_for_backward(s, t, out)
        else:
            ctx.save_for_backward(s, t, out, w)
        ctx.meta = (B, C, HW, float(thr))
        loss, cm = out[0], out[1]
        ctx.mark_non_differentiable(cm)
        ctx.set_materialize_grads(False)   # no zero-filled gradient for the cm output (a framework fill kernel)
        return loss, cm

    @staticmethod
    def backward(ctx, g_loss, g_cm):
        s, t, out = ctx.saved_tensors[:3]
        w = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        B, C, HW, thr = ctx.meta
        gs = torch.empty_like(s)
        g = _c(g_loss.float())
        N.call('ssseg_consistency_sm_bwd', N.dev_ptr(s), N.dev_ptr(t), N.dev_ptr(w), B, C, HW, thr, N.dev_ptr(out),
               N.dev_ptr(g), N.dev_ptr(gs), N.stream())
        return gs, None, None, None


def consistency_loss_softmax(student_logits, teacher_logits, thr, w=None):
    """The consistency loss over mutually exclusive classes: train.py:97-108 with the softmax lines (:97, :99) in
    place of the sigmoid ones.  [B,C,H,W] logits, 1 <= C <= 64; w [B,H,W] (optional, a constant) multiplies the
    confidence modulator like consistency_loss_weighted.  Returns (loss, sum(cm w) / npix); the loss is NaN when no
    weighted pixel is confident."""
    s, t = student_logits, teacher_logits
    if s.dim() < 3 or tuple(s.shape) != tuple(t.shape):
        raise ValueError(f'consistency_loss_softmax: student and teacher logits must have one shape [B,C,H,W], got '
                         f'{tuple(s.shape)} and {tuple(t.shape)}')
    if s.shape[1] > 64:
        raise ValueError(f'consistency_loss_softmax: {s.shape[1]} channels (at most 64 are supported)')
    if w is not None and w.numel() != s.shape[0] * s[0, 0].numel():
        raise ValueError('consistency_loss_softmax: w must hold one weight per pixel, [B, H, W]')
    _device_checked('consistency_loss_softmax', student=s, teacher=t, w=w)
    return _ConsistencySoftmax.apply(s, t, thr, w)


CE_WEIGHTINGS = {'pixel': 0, 'batch': 1}


class _ConsistencyCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, t, thr, w, weighting):
        s, t = _c(s.float()), _c(t.float())
        B, C = s.shape[:2]
        HW = s[0, 0].numel()
        out = torch.empty(4, device=s.device, dtype=torch.float32)
        nb = N.lib().ssseg_consistency_ce_workspace_bytes(B * HW)
        ws = N.workspace(nb, s.device)
        if w is not None:
            w = _c(w.float())
        # a [C] device tensor is one threshold per class (the _cls entry points); anything else is the scalar
        cls = isinstance(thr, torch.Tensor)
        if cls:
            N.call('ssseg_consistency_ce_cls_fwd', N.dev_ptr(s, 'student'), N.dev_ptr(t, 'teacher'), N.dev_ptr(w, 'w'),
                   B, C, HW, N.dev_ptr(thr, 'thr'), weighting, N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        else:
            N.call('ssseg_consistency_ce_fwd', N.dev_ptr(s, 'student'), N.dev_ptr(t, 'teacher'), N.dev_ptr(w, 'w'), B,
                   C, HW, float(thr), weighting, N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        if w is None:
            ctx.save_for_backward(s, t, out)
        else:
            ctx.save_for_backward(s, t, out, w)
        # (the threshold vector is a constant that is not an output: kept as it is, like the scalar)
        ctx.meta = (B, C, HW, thr if cls else float(thr), weighting)
        loss, cm = out[0], out[1]
        ctx.mark_non_differentiable(cm)
        ctx.set_materialize_grads(False)   # no zero-filled gradient for the cm output (a framework fill kernel)
        return loss, cm

    @staticmethod
    def backward(ctx, g_loss, g_cm):
        s, t, out = ctx.saved_tensors[:3]
        w = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        B, C, HW, thr, weighting = ctx.meta
        gs = torch.empty_like(s)
        g = _c(g_loss.float())
        if isinstance(thr, torch.Tensor):
            N.call('ssseg_consistency_ce_cls_bwd', N.dev_ptr(s), N.dev_ptr(t), N.dev_ptr(w), B, C, HW, N.dev_ptr(thr),
                   weighting, N.dev_ptr(out), N.dev_ptr(g), N.dev_ptr(gs), N.stream())
        else:
            N.call('ssseg_consistency_ce_bwd', N.dev_ptr(s), N.dev_ptr(t), N.dev_ptr(w), B, C, HW, thr, weighting,
                   N.dev_ptr(out), N.dev_ptr(g), N.dev_ptr(gs), N.stream())
        return gs, None, None, None, None


def consistency_loss_ce(student_logits, teacher_logits, thr, w=None, weighting='pixel'):
    """Pseudo-label consistency: cross-entropy of the student against the teacher's hard label y = argmax_c t_c,
    weighted by the teacher's confidence cm = [max_c softmax(t) > thr] (the teacher gets no gradient).  [B,C,H,W]
    logits, 1 <= C <= 64; w [B,H,W] (optional, a constant) weighs the pixels.  thr is a Python float, or a [C] float32
    tensor on the logits' device holding one threshold per class, read at the teacher's label: cm = [conf > thr[y]]
    (AdaptiveThreshold.update returns one; it is read when the kernels run, in the backward pass too).
    weighting='pixel' (FixMatch, CutMix-Seg): sum(w cm ce) / sum(w), the unconfident pixels selected out -- exactly 0.0,
    not NaN, when no pixel is confident;  'batch' (ClassMix): (sum(w cm) / sum(w)) * (sum(w ce) / sum(w)), the
    confident fraction a constant.  Returns (loss, sum(w cm) / npix); the loss is NaN only when sum(w) == 0."""
    s, t = student_logits, teacher_logits
    if weighting not in CE_WEIGHTINGS:
        raise ValueError(f"consistency_loss_ce: weighting must be 'pixel' or 'batch', got {weighting!r}")
    if s.dim() < 3 or tuple(s.shape) != tuple(t.shape):
        raise ValueError(f'consistency_loss_ce: student and teacher logits must have one shape [B,C,H,W], got '
                         f'{tuple(s.shape)} and {tuple(t.shape)}')
    if s.shape[1] > 64:
        raise ValueError(f'consistency_loss_ce: {s.shape[1]} channels (at most 64 are supported)')
    if w is not None and w.numel() != s.shape[0] * s[0, 0].numel():
        raise ValueError('consistency_loss_ce: w must hold one weight per pixel, [B, H, W]')
    cls = isinstance(thr, torch.Tensor)
    if cls and (thr.dim() != 1 or thr.numel() != s.shape[1] or thr.dtype != torch.float32 or not thr.is_contiguous()):
        raise ValueError(f'consistency_loss_ce: a threshold tensor must be a contiguous float32 vector of '
                         f'{s.shape[1]} entries (one per class), got {tuple(thr.shape)} {thr.dtype}')
    _device_checked('consistency_loss_ce', student=s, teacher=t, w=w)
    if cls:
        if thr.device != s.device:
            raise ValueError(f'consistency_loss_ce: the threshold vector is on {thr.device}, the logits on {s.device}')
        thr = thr.detach()
    return _ConsistencyCE.apply(s, t, thr, w, CE_WEIGHTINGS[weighting])


class AdaptiveThreshold:
    """Self-adaptive per-class confidence thresholds (FreeMatch: Wang et al., ICLR 2023, section 3.2, eqs. 5-8) for
    consistency_loss_ce.  The state -- tau, the EMA of the teacher's mean confidence, ptilde[C], the EMA of its class
    marginals, and the number of updates -- is fp64 on the device and is updated by one kernel sequence per step
    (ssseg_adaptive_thr_update: no host sync, graph-capturable); tau = ptilde_c = 1 / C at the start.
    update(teacher_logits) performs  tau <- m tau + (1 - m) mean max_c softmax(t),  ptilde_c <- m ptilde_c + (1 - m)
    mean softmax(t)_c  over all pixels of the batch and returns thr_c = ptilde_c / max_k ptilde_k * tau as a [C] float32
    device tensor -- the same storage at every call, overwritten by the next.  The device state is allocated at the
    first update, from that teacher's C and device: an eager step, before any capture.  Under data parallelism every
    rank's state follows its own batches (no collective)."""

    def __init__(self, momentum=0.999, num_classes=None):
        self.momentum = self._checked_momentum(momentum)
        self.state = self.thr = None           # device: [2 C + 3] fp64 (include/ssseg.h), [C] fp32
        self._host = None                      # (tau, ptilde, steps) while there is no device state
        if num_classes is not None:
            if not 1 <= int(num_classes) <= 64:
                raise ValueError(f'AdaptiveThreshold: {num_classes} classes (1 to 64 are supported)')
            self._host = self._initial(int(num_classes))

    @staticmethod
    def _checked_momentum(momentum):
        momentum = float(momentum)
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f'AdaptiveThreshold: momentum must be in [0, 1), got {momentum!r}')
        return momentum

    @staticmethod
    def _initial(C):
        return 1.0 / C, [1.0 / C] * C, 0

    @property
    def num_classes(self):
        if self.thr is not None:
            return self.thr.numel()
        return len(self._host[1]) if self._host is not None else None

    def _upload(self, tau, ptilde, steps):
        C = len(ptilde)
        host = torch.tensor([tau] + list(ptilde) + [float(steps)] + [0.0] * (C + 1), dtype=torch.float64)
        self.state.copy_(host)
        # thr_c of the state as it stands (the rule's expression, in fp64, rounded once)
        pt = host[1:C + 1]
        self.thr.copy_(((pt / pt.max()) * host[0]).float())

    def _allocate(self, C, device):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('AdaptiveThreshold: the first update allocates the state and must run eagerly, '
                               'before the step is captured')
        if self._host is not None and len(self._host[1]) != C:
            raise ValueError(f'AdaptiveThreshold: the state holds {len(self._host[1])} classes, the teacher has {C}')
        self.state = torch.empty(2 * C + 3, dtype=torch.float64, device=device)
        self.thr = torch.empty(C, dtype=torch.float32, device=device)
        self._upload(*(self._host or self._initial(C)))
        self._host = None

    def update(self, teacher_logits):
        t = teacher_logits
        if t.dim() < 3 or not 1 <= t.shape[1] <= 64:
            raise ValueError(f'AdaptiveThreshold.update: teacher logits must be [B,C,H,W] with 1 <= C <= 64, got '
                             f'{tuple(t.shape)}')
        _device_checked('AdaptiveThreshold.update', teacher=t)
        t = _c(t.detach().float())
        B, C = t.shape[:2]
        HW = t[0, 0].numel()
        if self.state is None:
            self._allocate(C, t.device)
        elif self.thr.numel() != C or self.thr.device != t.device:
            raise ValueError(f'AdaptiveThreshold.update: the state holds {self.thr.numel()} classes on '
                             f'{self.thr.device}, the teacher has {C} on {t.device}')
        nb = N.lib().ssseg_adaptive_thr_workspace_bytes(C)
        ws = N.workspace(nb, t.device)
        N.call('ssseg_adaptive_thr_update', N.dev_ptr(t, 'teacher'), B, C, HW, self.momentum, N.dev_ptr(self.state),
               N.dev_ptr(self.thr), N.dev_ptr(ws), nb, N.stream())
        return self.thr

    def reset(self):
        """back to tau = ptilde_c = 1 / C and no update taken (the device tensors stay the same storage)"""
        if self.state is not None:
            self._upload(*self._initial(self.thr.numel()))
        elif self._host is not None:
            self._host = self._initial(len(self._host[1]))

    def tau(self):
        """the current tau as a Python float (a host sync where the state is on the device: for logging points)"""
        if self.state is not None:
            return float(self.state[0])
        return self._host[0] if self._host is not None else None

    def state_dict(self):
        """host copies: {'tau': float, 'ptilde': [C floats], 'steps': int} ({} before the class count is known)"""
        if self.state is not None:
            C = self.thr.numel()
            host = self.state[:C + 2].cpu().tolist()
            return {'tau': host[0], 'ptilde': host[1:C + 1], 'steps': int(host[C + 1])}
        if self._host is None:
            return {}
        return {'tau': self._host[0], 'ptilde': list(self._host[1]), 'steps': self._host[2]}

    def load_state_dict(self, sd):
        if not sd:
            return
        tau, ptilde, steps = float(sd['tau']), [float(v) for v in sd['ptilde']], int(sd['steps'])
        C = self.num_classes
        if C is not None and len(ptilde) != C:
            raise ValueError(f'AdaptiveThreshold.load_state_dict: the state dict holds {len(ptilde)} classes, this '
                             f'object {C}')
        if not 1 <= len(ptilde) <= 64:
            raise ValueError(f'AdaptiveThreshold.load_state_dict: {len(ptilde)} classes (1 to 64 are supported)')
        if self.state is not None:
            self._upload(tau, ptilde, steps)
        else:
            self._host = (tau, ptilde, steps)


# ------------------------------------------------------------------------------------------------
# EMA / optimiser over flat arenas
# ------------------------------------------------------------------------------------------------
def ema_update_(ema_flat, param_flat, alpha):
    """mean_teacher.update_ema_variables parameter loop (mean_teacher.py:10-11), one launch."""
    assert ema_flat.numel() == param_flat.numel() and ema_flat.dtype == torch.float32
    N.call('ssseg_ema_update', N.dev_ptr(ema_flat, 'ema'), N.dev_ptr(param_flat, 'param'), ema_flat.numel(),
           float(alpha), N.stream())


def sqnorm_(x_flat, out):
    nb = N.lib().ssseg_reduce_workspace_bytes(x_flat.numel())
    ws = N.workspace(nb, x_flat.device)
    N.call('ssseg_sqnorm_accum', N.dev_ptr(x_flat, 'x'), x_flat.numel(), N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())


def sgd_step_(param, grad, buf, shadow, lr, momentum, wd, max_norm, sqnorm, first, amp_state=None):
    N.call('ssseg_sgd_step', N.dev_ptr(param, 'param'), N.dev_ptr(grad, 'grad'),
           N.dev_ptr(buf) if buf is not None else None, N.dev_ptr(shadow) if shadow is not None else None,
           param.numel(), float(lr), float(momentum), float(wd), float(max_norm),
           N.dev_ptr(sqnorm) if sqnorm is not None else None, int(bool(first)),
           N.dev_ptr(amp_state) if amp_state is not None else None, N.stream())


def optim_prepare_(state, mode, lr, beta1, beta2, wd, max_norm, k=1, nsma_threshold=0.0, sqnorm=None, amp_state=None):
    """Per-step scalars of the fused Adam family (step counter, clip / unscale, bias corrections, Ranger's
    decisions) computed on the device into `state` (fp64, native.OPT_STATE_DOUBLES)."""
    assert state.dtype == torch.float64 and state.numel() >= N.OPT_STATE_DOUBLES
    N.call('ssseg_optim_prepare', N.dev_ptr(state, 'state'), int(mode), float(lr), float(beta1), float(beta2),
           float(wd), float(max_norm), int(k), float(nsma_threshold),
           N.dev_ptr(sqnorm) if sqnorm is not None else None,
           N.dev_ptr(amp_state) if amp_state is not None else None, N.stream())


def optim_step_(param, grad, exp_avg, exp_avg_sq, exp_avg_lr, previous_grad, slow_buffer, mode, version, beta1, beta2,
                beta3, eps, wd, alpha, state):
    """One pass of the fused Adam-family update over the flat arenas, from the scalars optim_prepare_ left."""
    N.call('ssseg_optim_step', N.dev_ptr(param, 'param'), N.dev_ptr(grad, 'grad'), N.dev_ptr(exp_avg, 'exp_avg'),
           N.dev_ptr(exp_avg_sq, 'exp_avg_sq'), N.dev_ptr(exp_avg_lr), N.dev_ptr(previous_grad),
           N.dev_ptr(slow_buffer), param.numel(), int(mode), int(version), float(beta1), float(beta2), float(beta3),
           float(eps), float(wd), float(alpha), N.dev_ptr(state, 'state'), N.stream())


# ------------------------------------------------------------------------------------------------
# Lovász (losses.py:239-250)
# ------------------------------------------------------------------------------------------------
class _Lovasz(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits, target = _c(logits.float()), _c(target.float())
        B, C = logits.shape[:2]
        HW = logits[0, 0].numel()
        out = torch.empty((), device=logits.device, dtype=torch.float32)
        nb = N.lib().ssseg_lovasz_workspace_bytes(B, HW)
        ws = N.workspace(nb, logits.device)
        N.call('ssseg_lovasz_fwd', N.dev_ptr(logits, 'logits'), N.dev_ptr(target, 'target'), B, C, HW,
               N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(logits, target)
        ctx.ws, ctx.nb = ws, nb   # the forward's per-pixel gradient and image scales: the backward does not re-sort
        return out

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved_tensors
        B, C = logits.shape[:2]
        HW = logits[0, 0].numel()
        gx = torch.empty_like(logits)
        g = _c(g.float())
        N.call('ssseg_lovasz_bwd_from_fwd', N.dev_ptr(logits), N.dev_ptr(target), B, C, HW, N.dev_ptr(g),
               N.dev_ptr(gx), N.dev_ptr(ctx.ws), ctx.nb, N.stream())
        # (ctx.ws stays for the lifetime of ctx: a second backward through a retained graph reads it again)
        return gx, None


def lovasz_binary(logits, target, valid_weighted=True):
    """binary_lovasz_loss_with_logits (losses.py:239-250) on the device.  valid_weighted=False is the plain
    lovasz_softmax(classes=[1], per_image=True) of its building block (lovasz.py:155-170): the mean over all images,
    through the general kernels with the dense target's argmax as the label."""
    if not valid_weighted:
        return lovasz_general(logits, target, N.LOVASZ_PROBAS, [1], per_image=True, dense_target=True)
    return _Lovasz.apply(logits, target)


# ------------------------------------------------------------------------------------------------
# General Lovász losses (lovasz.py:79-127, 155-220): csrc/lovasz.hip, ssseg_lovasz_gen_*
# ------------------------------------------------------------------------------------------------
class _LovaszGen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, cfg):
        kind, mode, per_image, present, classes, ignore = cfg
        B, C = x.shape[:2]
        HW = x[0, 0].numel()
        sel = (ctypes.c_int64 * len(classes))(*classes)
        args = (kind, B, C, HW, mode, int(per_image), int(present), sel, len(classes), int(ignore is not None),
                int(ignore) if ignore is not None else 0)
        nb = N.lib().ssseg_lovasz_gen_workspace_bytes(B, C, HW, int(per_image), len(classes))
        if nb == 0:
            raise ValueError(f'lovasz: input {tuple(x.shape)} with {len(classes)} classes, per_image={per_image} is '
                             'outside the kernels\' bounds (1 <= C <= 64, at most 2^24 pixels per group, '
                             'groups * classes <= 65535)')
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws = N.workspace(nb, x.device)
        N.call('ssseg_lovasz_gen_fwd', N.dev_ptr(x, 'input'), N.dev_ptr(labels, 'labels'), *args, N.dev_ptr(out),
               N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, labels)
        ctx.args, ctx.ws, ctx.nb = args, ws, nb   # the forward's per-pixel weights and class scales: no second sort
        return out

    @staticmethod
    def backward(ctx, g):
        x, labels = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_lovasz_gen_bwd_from_fwd', N.dev_ptr(x), N.dev_ptr(labels), *ctx.args, N.dev_ptr(g),
               N.dev_ptr(gx), N.dev_ptr(ctx.ws), ctx.nb, N.stream())
        # (ctx.ws stays for the lifetime of ctx: a second backward through a retained graph reads it again)
        return gx, None, None


def lovasz_label_kind(labels):
    """(labels as the kernels read them in place, SSSEG_LOVASZ_LABEL_* code); other integer types become int64"""
    if labels.dtype == torch.uint8:
        return _c(labels), N.LOVASZ_LABEL_U8
    if labels.dtype == torch.float32:
        return _c(labels), N.LOVASZ_LABEL_F32
    if labels.dtype.is_floating_point:
        return _c(labels.float()), N.LOVASZ_LABEL_F32
    return _c(labels.long()), N.LOVASZ_LABEL_I64


def lovasz_general(x, labels, mode, classes, per_image=False, ignore=None, present=False, dense_target=False):
    """The Lovász family on the device.  x [B, C, ...] f32: probabilities (LOVASZ_PROBAS), logits with the softmax
    fused (LOVASZ_SOFTMAX) or one-channel hinge logits (LOVASZ_HINGE).  labels [B, ...] (int64 / uint8 / float
    values), or with dense_target a [B, C, ...] target whose argmax is the label.  classes: list of class ids;
    present: count only those with a foreground pixel in the group.  Returns the scalar loss (differentiable in x)."""
    if x.dim() < 3:
        raise ValueError(f'lovasz: expected input [B, C, ...], got {tuple(x.shape)}')
    x = _c(x.float())
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    classes = [int(c) for c in classes]
    if not classes:
        raise ValueError('lovasz: `classes` is empty')
    if not 1 <= C <= 64:
        raise ValueError(f'lovasz: {C} channels (the kernels cover 1 <= C <= 64)')
    if len(classes) > 64:
        raise ValueError(f'lovasz: {len(classes)} classes selected (the kernels cover at most 64)')
    if C == 1 and len(classes) != 1:
        raise ValueError('Sigmoid output possible only with 1 class')
    if C > 1 and not all(0 <= c < C for c in classes):
        raise ValueError(f'lovasz: classes {classes} outside [0, {C})')
    if dense_target:
        if tuple(labels.shape) != tuple(x.shape):
            raise ValueError(f'lovasz: input {tuple(x.shape)} and dense target {tuple(labels.shape)} must have the '
                             'same shape')
        if C < 2:
            raise ValueError('lovasz: a dense target needs at least two channels')
        labels, kind = _c(labels.float()), N.LOVASZ_LABEL_DENSE
    else:
        if labels.numel() != B * HW:
            raise ValueError(f'lovasz: labels {tuple(labels.shape)} do not hold one label per pixel of '
                             f'{tuple(x.shape)}')
        labels, kind = lovasz_label_kind(labels)
    return _LovaszGen.apply(x, labels, (kind, int(mode), bool(per_image), bool(present), tuple(classes), ignore))


# ------------------------------------------------------------------------------------------------
# RMILoss (losses.py:271-592, sigmoid form)
# ------------------------------------------------------------------------------------------------
class _RMI(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, geo):
        logits, target = _c(logits.float()), _c(target.float())
        Nn, C, H, W = logits.shape
        nb = N.lib().ssseg_rmi_workspace_bytes(Nn, C, H, W, *geo)
        if nb == 0:
            raise ValueError(f'RMILoss: geometry {tuple(logits.shape)} / (num_classes, radius, k, s, pad) = {geo} '
                             'is not supported')
        # the workspace carries the pooled maps and the backward coefficients to backward: a tensor of its own
        ws = torch.empty(nb, dtype=torch.uint8, device=logits.device)
        out = torch.empty((), device=logits.device, dtype=torch.float32)
        want = int(ctx.needs_input_grad[0])
        N.call('ssseg_rmi_fwd', N.dev_ptr(logits, 'logits'), N.dev_ptr(target, 'target'), Nn, C, H, W, *geo, want,
               N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        if want:
            ctx.save_for_backward(logits, ws)
        ctx.geo = geo
        return out

    @staticmethod
    def backward(ctx, g):
        logits, ws = ctx.saved_tensors
        Nn, C, H, W = logits.shape
        gx = torch.empty_like(logits)
        g = _c(g.float())
        N.call('ssseg_rmi_bwd', N.dev_ptr(logits), Nn, C, H, W, *ctx.geo, N.dev_ptr(g), N.dev_ptr(gx), N.dev_ptr(ws),
               ws.numel(), N.stream())
        return gx, None, None


def rmi_loss(logits, target, num_classes, radius, pool_k, pool_s, pool_pad):
    """RMILoss.forward (losses.py:480-592) on the device: sigmoid probabilities, avg pool (k, s, pad; (1, 1, 0) =
    none), fp64 region covariances and Cholesky log-det per (image, class), summed over classes."""
    if logits.dim() != 4 or tuple(logits.shape) != tuple(target.shape):
        raise ValueError(f'RMILoss: logits {tuple(logits.shape)} and target {tuple(target.shape)} must be the same NCHW shape')
    return _RMI.apply(logits, target, (int(num_classes), int(radius), int(pool_k), int(pool_s), int(pool_pad)))


# ------------------------------------------------------------------------------------------------
# The other reference losses (csrc/seglosses.hip): CE, OHEM, Focal, NormalizedFocal, Dice, entropies
# ------------------------------------------------------------------------------------------------
def _bchw(x, name):
    if x.dim() < 3:
        raise ValueError(f'{name}: expected [B, C, ...], got {tuple(x.shape)}')
    B, C = x.shape[:2]
    if not 1 <= C <= 64:
        raise ValueError(f'{name}: {C} channels (the kernels cover 1 <= C <= 64)')
    return B, C, x[0, 0].numel()


def _seg_ws(kind, B, C, HW, device):
    nb = N.lib().ssseg_segloss_workspace_bytes(kind, B, C, HW)
    return N.workspace(nb, device), nb


def _same_shape(x, t, name):
    if tuple(x.shape) != tuple(t.shape):
        raise ValueError(f'{name}: input {tuple(x.shape)} and target {tuple(t.shape)} must have the same shape')


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, red):
        x, t = _c(x.float()), _c(t.float())
        B, C, HW = _bchw(x, 'DenseCrossEntropyLossWithLogits')
        if red == N.RED_MEAN:
            out = torch.empty((), device=x.device, dtype=torch.float32)
        else:
            out = torch.empty((B,) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
        ws, nb = _seg_ws(N.LOSS_REDUCE, B, C, HW, x.device)
        N.call('ssseg_ce_fwd', N.dev_ptr(x, 'input'), N.dev_ptr(t, 'target'), B, C, HW, red, N.dev_ptr(out),
               N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t)
        ctx.meta = (B, C, HW, red)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        B, C, HW, red = ctx.meta
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_ce_bwd', N.dev_ptr(x), N.dev_ptr(t), B, C, HW, red, N.dev_ptr(g), N.dev_ptr(gx), N.stream())
        return gx, None, None


def dense_cross_entropy(x, t, reduction='mean'):
    """DenseCrossEntropyLossWithLogits.forward (losses.py:30-39): -(t * log_softmax(x, 1)).sum(1), mean or none."""
    _same_shape(x, t, 'DenseCrossEntropyLossWithLogits')
    return _CE.apply(x, t, {'mean': N.RED_MEAN, 'none': N.RED_NONE}[reduction])


class _Ohem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, thresh, min_kept):
        x, t = _c(x.float()), _c(t.float())
        B, C, HW = _bchw(x, 'OhemCrossEntropy')
        out = torch.empty((), device=x.device, dtype=torch.float32)
        # the workspace carries pred per pixel, the threshold and the kept count to the backward: a tensor of its own
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_OHEM, B, C, HW)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        N.call('ssseg_ohem_fwd', N.dev_ptr(x, 'logits'), N.dev_ptr(t, 'target'), B, C, HW, float(thresh),
               int(min_kept), N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t, ws)
        ctx.meta = (B, C, HW)
        ctx.mark_non_differentiable(ws)
        ctx.set_materialize_grads(False)
        return out, ws

    @staticmethod
    def backward(ctx, g, g_ws):
        x, t, ws = ctx.saved_tensors
        B, C, HW = ctx.meta
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_ohem_bwd', N.dev_ptr(x), N.dev_ptr(t), B, C, HW, N.dev_ptr(g), N.dev_ptr(gx), N.dev_ptr(ws),
               ws.numel(), N.stream())
        return gx, None, None, None


def ohem_cross_entropy(x, t, thresh, min_kept, return_state=False):
    """OhemCrossEntropy.forward (losses.py:58-69).  return_state: also (threshold, kept count), a float64 [2] device
    view of the forward's workspace."""
    _same_shape(x, t, 'OhemCrossEntropy')
    out, ws = _Ohem.apply(x, t, thresh, min_kept)
    if return_state:
        return out, ws[:16].view(torch.float64)
    return out


def _label_map(x, labels, name):
    """(B, C, HW, labels as the kernels read them in place, label-kind code) of logits [B, C, ...] and a label map
    with one label per pixel: uint8 stays, every other integer type becomes int64"""
    if x.dim() < 3:
        raise ValueError(f'{name}: expected logits [B, C, ...], got {tuple(x.shape)}')
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    if not 2 <= C <= 64:
        raise ValueError(f'{name}: {C} channels (the label-map kernels cover 2 <= C <= 64)')
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f'{name}: the label map must be uint8 or int64, got {labels.dtype}')
    if labels.dim() != x.dim() - 1 or labels.shape[0] != B or tuple(labels.shape[1:]) != tuple(x.shape[2:]):
        raise ValueError(f'{name}: labels {tuple(labels.shape)} do not hold one label per pixel of {tuple(x.shape)}')
    if labels.dtype == torch.uint8:
        return B, C, HW, _c(labels), N.LOVASZ_LABEL_U8
    return B, C, HW, _c(labels.long()), N.LOVASZ_LABEL_I64


class _CELabels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, weight, args):
        kind, B, C, HW, ignore, red, eps, empty_zero = args
        if red == N.RED_NONE:
            out = torch.empty((B,) + tuple(x.shape[2:]), device=x.device, dtype=torch.float32)
        else:
            out = torch.empty((), device=x.device, dtype=torch.float32)
        # the workspace carries the 'mean' denominator to the backward: a tensor of its own
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_CE_LABELS, B, C, HW)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        N.call('ssseg_ce_labels_fwd', N.dev_ptr(x, 'input'), N.dev_ptr(labels, 'labels'), kind, B, C, HW,
               N.dev_ptr(weight, 'weight'), ignore, eps, red, empty_zero, N.dev_ptr(out), N.dev_ptr(ws), nb,
               N.stream())
        ctx.save_for_backward(x, labels, weight, ws)
        ctx.args = args
        return out

    @staticmethod
    def backward(ctx, g):
        x, labels, weight, ws = ctx.saved_tensors
        kind, B, C, HW, ignore, red, eps, _ = ctx.args
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_ce_labels_bwd', N.dev_ptr(x), N.dev_ptr(labels), kind, B, C, HW, N.dev_ptr(weight), ignore, eps,
               red, N.dev_ptr(g), N.dev_ptr(gx), N.dev_ptr(ws), ws.numel(), N.stream())
        return gx, None, None, None


def cross_entropy_labels(x, labels, weight=None, ignore_index=255, reduction='mean', label_smoothing=0.0,
                         empty='nan'):
    """F.cross_entropy(x, labels, weight, ignore_index=..., reduction=..., label_smoothing=...) on the device.
    x [B, C, ...] f32 logits, 2 <= C <= 64; labels [B, ...] uint8 or int64, read in place.  ignore_index may lie
    inside [0, C).  A label outside [0, C) that is not ignore_index is void as well: the kernels select the labelled
    channel by comparison and nothing is checked on the host (that would be a sync).  'mean' divides by the sum of
    w_y over the valid pixels; with everything void it is NaN like torch (empty='nan') or 0 (empty='zero'), and the
    gradient is all zeros either way."""
    name = 'cross_entropy_labels'
    if reduction not in ('mean', 'sum', 'none'):
        raise ValueError(f'{name}: {reduction} is not a valid value for reduction')
    if empty not in ('nan', 'zero'):
        raise ValueError(f"{name}: empty must be 'nan' or 'zero', got {empty!r}")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f'{name}: label_smoothing {label_smoothing} outside [0, 1)')
    B, C, HW, labels, kind = _label_map(x, labels, name)
    if weight is not None:
        if weight.numel() != C:
            raise ValueError(f'{name}: weight holds {weight.numel()} values for {C} classes')
        weight = _c(weight.float()).reshape(C)
    red = {'none': N.RED_NONE, 'mean': N.RED_MEAN, 'sum': N.RED_SUM}[reduction]
    return _CELabels.apply(_c(x.float()), labels, weight,
                           (kind, B, C, HW, int(ignore_index), red, float(label_smoothing), int(empty == 'zero')))


class _OhemLabels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, args):
        kind, B, C, HW, ignore, thresh, min_kept = args
        out = torch.empty((), device=x.device, dtype=torch.float32)
        # pred per pixel, the threshold and the kept count go to the backward in the workspace: a tensor of its own
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_OHEM_LABELS, B, C, HW)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        N.call('ssseg_ohem_labels_fwd', N.dev_ptr(x, 'logits'), N.dev_ptr(labels, 'labels'), kind, B, C, HW, ignore,
               thresh, min_kept, N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, labels, ws)
        ctx.meta = (kind, B, C, HW)
        ctx.mark_non_differentiable(ws)
        ctx.set_materialize_grads(False)
        return out, ws

    @staticmethod
    def backward(ctx, g, g_ws):
        x, labels, ws = ctx.saved_tensors
        kind, B, C, HW = ctx.meta
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_ohem_labels_bwd', N.dev_ptr(x), N.dev_ptr(labels), kind, B, C, HW, N.dev_ptr(g), N.dev_ptr(gx),
               N.dev_ptr(ws), ws.numel(), N.stream())
        return gx, None, None


def ohem_cross_entropy_labels(x, labels, thresh, min_kept, ignore_label=255, return_state=False):
    """OhemCrossEntropy on a label map [B, ...] (uint8 / int64) with a void label, as in the HRNet original: the
    order statistic (k = min(min_kept, n_valid - 1)), the threshold and the mean run over the valid pixels only.
    Labels outside [0, C) are void like ignore_label.  No valid pixel: NaN loss, zero gradient.  return_state: also
    (threshold, kept count), a float64 [2] device view of the forward's workspace."""
    name = 'ohem_cross_entropy_labels'
    if int(min_kept) < 0:
        raise ValueError(f'{name}: min_kept {min_kept} is negative')
    B, C, HW, labels, kind = _label_map(x, labels, name)
    out, ws = _OhemLabels.apply(_c(x.float()), labels,
                                (kind, B, C, HW, int(ignore_label), float(thresh), int(min_kept)))
    if return_state:
        return out, ws[:16].view(torch.float64)
    return out


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, alpha, gamma):
        x, t = _c(x.float()), _c(t.float())
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws, nb = _seg_ws(N.LOSS_REDUCE, 1, 1, x.numel(), x.device)
        N.call('ssseg_focal_fwd', N.dev_ptr(x, 'inputs'), N.dev_ptr(t, 'targets'), x.numel(), alpha, gamma,
               N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t)
        ctx.meta = (alpha, gamma)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_focal_bwd', N.dev_ptr(x), N.dev_ptr(t), x.numel(), *ctx.meta, N.dev_ptr(g), N.dev_ptr(gx),
               N.stream())
        return gx, None, None, None


def focal_loss(x, t, alpha, gamma):
    """FocalLoss.forward (losses.py:79-90)."""
    _same_shape(x, t, 'FocalLoss')
    return _Focal.apply(x, t, float(alpha), float(gamma))


class _NFL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, label, params, k_sum):
        x, label = _c(x.float()), _c(label.float())
        B, C, HW = _bchw(x, 'NormalizedFocalLossSigmoid')
        out = torch.empty(B, device=x.device, dtype=torch.float32)
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_NFL, B, C, HW)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)   # mult and the denominators stay for the backward
        N.call('ssseg_nfl_fwd', N.dev_ptr(x, 'pred'), N.dev_ptr(label, 'label'), B, C, HW, ctypes.addressof(params),
               N.dev_ptr(out), N.dev_ptr(k_sum) if k_sum is not None else None, N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, label, ws)
        ctx.meta = (B, C, HW, params)
        return out

    @staticmethod
    def backward(ctx, g):
        x, label, ws = ctx.saved_tensors
        B, C, HW, params = ctx.meta
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_nfl_bwd', N.dev_ptr(x), N.dev_ptr(label), B, C, HW, ctypes.addressof(params), N.dev_ptr(g),
               N.dev_ptr(gx), N.dev_ptr(ws), ws.numel(), N.stream())
        return gx, None, None, None


def normalized_focal_loss(pred, label, params, k_sum=None):
    """NormalizedFocalLossSigmoid.forward (losses.py:115-151) -> [B]; k_sum (1 float, device) is updated in place."""
    _same_shape(pred, label, 'NormalizedFocalLossSigmoid')
    return _NFL.apply(pred, label, params, k_sum)


class _DiceLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        x, t = _c(x.float()), _c(t.float())
        B, C, HW = _bchw(x, 'DiceWithLogitsLoss')
        out = torch.empty((), device=x.device, dtype=torch.float32)
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_DICE_LOGITS, B, C, HW)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)   # the per-(b,c) backward coefficients
        N.call('ssseg_dice_logits_fwd', N.dev_ptr(x, 'input'), N.dev_ptr(t, 'target'), B, C, HW, N.dev_ptr(out),
               N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t, ws)
        ctx.meta = (B, C, HW)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t, ws = ctx.saved_tensors
        B, C, HW = ctx.meta
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_dice_logits_bwd', N.dev_ptr(x), N.dev_ptr(t), B, C, HW, N.dev_ptr(g), N.dev_ptr(gx),
               N.dev_ptr(ws), ws.numel(), N.stream())
        return gx, None


def dice_with_logits(x, t):
    """DiceWithLogitsLoss.forward (losses.py:159-167)."""
    _same_shape(x, t, 'DiceWithLogitsLoss')
    return _DiceLogits.apply(x, t)


class _DiceProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, log_mode, gamma):
        p, t = _c(p.float()), _c(t.float())
        B = p.shape[0]
        n = p[0].numel()
        out = torch.empty(B, device=p.device, dtype=torch.float32)
        nb = N.lib().ssseg_segloss_workspace_bytes(N.LOSS_DICE_PROB, B, 1, n)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)   # per-sample numerator and denominator
        N.call('ssseg_dice_prob_fwd', N.dev_ptr(p, 'input'), N.dev_ptr(t, 'target'), B, n, log_mode, gamma,
               N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(t, ws)
        ctx.meta = (B, n, log_mode, gamma)
        return out

    @staticmethod
    def backward(ctx, g):
        t, ws = ctx.saved_tensors
        B, n, log_mode, gamma = ctx.meta
        gx = torch.empty_like(t)
        g = _c(g.float())
        N.call('ssseg_dice_prob_bwd', N.dev_ptr(t), B, n, log_mode, gamma, N.dev_ptr(g), N.dev_ptr(gx),
               N.dev_ptr(ws), ws.numel(), N.stream())
        return gx, None, None, None


def dice_prob(p, t, log_mode=False, gamma=1.0):
    """dice_loss / log_dice_loss (losses.py:221-236) on probabilities -> [B]."""
    _same_shape(p, t, 'dice_loss')
    return _DiceProb.apply(p, t, int(bool(log_mode)), float(gamma))


class _BinaryEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x.float())
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws, nb = _seg_ws(N.LOSS_REDUCE, 1, 1, x.numel(), x.device)
        N.call('ssseg_binary_entropy_fwd', N.dev_ptr(x, 'input'), x.numel(), N.dev_ptr(out), N.dev_ptr(ws), nb,
               N.stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_binary_entropy_bwd', N.dev_ptr(x), x.numel(), N.dev_ptr(g), N.dev_ptr(gx), N.stream())
        return gx


def binary_entropy(x):
    """binary_entropy_loss (losses.py:253-257)."""
    return _BinaryEntropy.apply(x)


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x.float())
        B, C, HW = _bchw(x, 'entropy_loss')
        out = torch.empty((), device=x.device, dtype=torch.float32)
        ws, nb = _seg_ws(N.LOSS_REDUCE, B, C, HW, x.device)
        N.call('ssseg_entropy_fwd', N.dev_ptr(x, 'input'), B, C, HW, N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x)
        ctx.meta = (B, C, HW)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_entropy_bwd', N.dev_ptr(x), *ctx.meta, N.dev_ptr(g), N.dev_ptr(gx), N.stream())
        return gx


def entropy(x):
    """entropy_loss (losses.py:260-264)."""
    return _Entropy.apply(x)


class _BCERed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, red):
        x, t = _c(x.float()), _c(t.float())
        out = torch.empty_like(x) if red == N.RED_NONE else torch.empty((), device=x.device, dtype=torch.float32)
        ws, nb = _seg_ws(N.LOSS_REDUCE, 1, 1, x.numel(), x.device)
        N.call('ssseg_bce_logits_red_fwd', N.dev_ptr(x, 'x'), N.dev_ptr(t, 'target'), x.numel(), red,
               N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
        ctx.save_for_backward(x, t)
        ctx.red = red
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = _c(g.float())
        N.call('ssseg_bce_logits_red_bwd', N.dev_ptr(x), N.dev_ptr(t), x.numel(), ctx.red, N.dev_ptr(g),
               N.dev_ptr(gx), N.stream())
        return gx, None, None


def bce_with_logits(x, t, reduction):
    """F.binary_cross_entropy_with_logits(x, t, reduction=...) (losses.py:47); 'mean' is the hot-path kernel."""
    if reduction == 'mean':
        return _BCE.apply(x, t)
    _same_shape(x, t, 'DenseBinaryCrossEntropyLossWithLogits')
    return _BCERed.apply(x, t, {'none': N.RED_NONE, 'sum': N.RED_SUM}[reduction])


def smooth_labels(t, alpha=0.1):
    """smooth_labels (losses.py:267-268): t * (1 - alpha) + alpha / C (no gradient: targets)."""
    x = _c(t.detach().float())
    out = torch.empty_like(x)
    N.call('ssseg_smooth_labels', N.dev_ptr(x, 'target'), N.dev_ptr(out), x.numel(), float(1 - alpha),
           float(alpha / t.size(1)), N.stream())
    return out


# ------------------------------------------------------------------------------------------------
# Multi-scale attention blend (multiscale_attention.py:52-54)
# ------------------------------------------------------------------------------------------------
class _AttBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lo, hi, att):
        Nn, C, H, W = hi.shape
        if tuple(lo.shape) != (Nn, C, H, W) or tuple(att.shape) != (Nn, 1, H, W):
            raise ValueError(f'att_blend: shapes {tuple(lo.shape)} {tuple(hi.shape)} {tuple(att.shape)}')
        for t, n in ((lo, 'lo'), (hi, 'hi'), (att, 'att')):
            if t.dtype != torch.float32:
                raise RuntimeError(f'att_blend: {n} must be fp32')
        out = torch.empty((Nn, C, H, W), device=hi.device, dtype=torch.float32)
        N.call('ssseg_att_blend_fwd', N.dev_ptr(lo, 'lo'), N.strides4(lo), N.dev_ptr(hi, 'hi'), N.strides4(hi),
               N.dev_ptr(att, 'att'), N.strides4(att), N.dev_ptr(out), Nn, C, H, W, N.stream())
        ctx.save_for_backward(lo, hi, att)
        return out

    @staticmethod
    def backward(ctx, g):
        lo, hi, att = ctx.saved_tensors
        Nn, C, H, W = hi.shape
        g = g.float()
        glo = torch.empty((Nn, C, H, W), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        ghi = torch.empty((Nn, C, H, W), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        gat = torch.empty((Nn, 1, H, W), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        N.call('ssseg_att_blend_bwd', N.dev_ptr(g), N.strides4(g), N.dev_ptr(lo), N.strides4(lo), N.dev_ptr(hi),
               N.strides4(hi), N.dev_ptr(att), N.strides4(att), N.dev_ptr(glo), N.dev_ptr(ghi), N.dev_ptr(gat), Nn, C,
               H, W, N.stream())
        return glo, ghi, gat


def att_blend(lo, hi, att_logits):
    """lo*sigmoid(a) + hi*(1-sigmoid(a)) (MultiscaleAttention, multiscale_attention.py:52-54); fp32 NCHW
    tensors of any strides, att [N,1,H,W] pre-sigmoid; returns contiguous NCHW."""
    return _AttBlend.apply(lo, hi, att_logits)


# ------------------------------------------------------------------------------------------------
# Validation metrics (train.validate, train.py:150-195)
# ------------------------------------------------------------------------------------------------
class SegMetrics:
    """Dice (metrics.dice_metric on the nearest-resized argmax one-hot, train.py:178-186) and the
    confusion counts of lovasz.iou (lovasz.py:54-73, C=2, per_image=False) in one pass per batch.
    `update(logits, mask)` returns a device tensor [dice_mean, iou0, iou1, miou]; the IoUs are over every
    batch seen so far (running counts on the device)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.total = torch.zeros(8, dtype=torch.int64, device=self.device)

    def update(self, logits, mask):
        if logits.dim() != 4 or logits.shape[1] != 2 or mask.dim() != 4 or mask.shape[1] != 2:
            raise ValueError('SegMetrics: binary [B,2,h,w] logits and [B,2,H,W] mask expected')
        if logits.shape[0] != mask.shape[0]:
            raise ValueError('SegMetrics: batch size mismatch')
        logits = logits if logits.dtype == torch.float32 else logits.float()
        mask = mask if mask.dtype == torch.float32 else mask.float()
        B, _, h, w = logits.shape
        H, W = mask.shape[2:]
        counts = torch.empty(B, 8, dtype=torch.int64, device=logits.device)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        N.call('ssseg_seg_metrics', N.dev_ptr(logits, 'logits'), N.strides4(logits), h, w, N.dev_ptr(mask, 'mask'),
               N.strides4(mask), B, H, W, N.dev_ptr(counts), N.dev_ptr(self.total), N.dev_ptr(out), N.stream())
        self.counts = counts
        return out


class SegMetricsMC:
    """SegMetrics for num_classes mutually exclusive classes (1 <= C <= 64): train.py:171-175 with num_classes = C
    (Dice of the nearest-resized argmax one-hot over channels 1..) and the confusion matrix of lovasz.iou
    (lovasz.py:54-73, per_image=False) in one pass per batch.  `update(logits, target)` takes [B,C,h,w] logits and
    either a dense [B,C,H,W] mask or a [B,H,W] int64 label map (pixels labelled `ignore` are left out of every count)
    and returns the device vector [dice_mean, mean IoU (a fraction), 100*IoU_0, ..., 100*IoU_{C-1}]; the IoUs are
    over every batch seen so far.  .total [C,C] is the running confusion matrix (rows label, columns prediction),
    .counts the last batch's, .dice its per-image [B,2] Dice numerators and denominators."""

    def __init__(self, device, num_classes, ignore=None):
        num_classes = int(num_classes)
        if not 1 <= num_classes <= 64:
            raise ValueError(f'SegMetricsMC: {num_classes} channels (1 to 64 are supported)')
        self.device = torch.device(device)
        self.num_classes = num_classes
        self.ignore = None if ignore is None else int(ignore)
        self.total = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=self.device)
        self.counts = self.dice = None

    def update(self, logits, target):
        C = self.num_classes
        if logits.dim() != 4 or logits.shape[1] != C:
            raise ValueError(f'SegMetricsMC: [B,{C},h,w] logits expected, got {tuple(logits.shape)}')
        labels = target.dim() == 3
        if labels:
            if target.dtype != torch.int64:
                raise ValueError('SegMetricsMC: a [B,H,W] label map must be int64')
        elif target.dim() != 4 or target.shape[1] != C:
            raise ValueError(f'SegMetricsMC: a [B,{C},H,W] mask or a [B,H,W] int64 label map expected, got '
                             f'{tuple(target.shape)}')
        if logits.shape[0] != target.shape[0]:
            raise ValueError('SegMetricsMC: batch size mismatch')
        _device_checked('SegMetricsMC', logits=logits, target=target)
        logits = logits if logits.dtype == torch.float32 else logits.float()
        if not labels:
            target = target if target.dtype == torch.float32 else target.float()
        B, _, h, w = logits.shape
        H, W = target.shape[-2:]
        counts = torch.empty(C, C, dtype=torch.int64, device=logits.device)
        dice = torch.empty(B, 2, dtype=torch.int64, device=logits.device)
        out = torch.empty(2 + C, dtype=torch.float32, device=logits.device)
        tstr = (ctypes.c_int64 * 4)(*(tuple(target.stride()) + (0,) * (4 - target.dim())))
        N.call('ssseg_seg_metrics_mc', N.dev_ptr(logits, 'logits'), N.strides4(logits), h, w,
               N.dev_ptr(target, 'target'), tstr, int(labels), int(self.ignore is not None),
               self.ignore if self.ignore is not None else 0, B, C, H, W, N.dev_ptr(counts), N.dev_ptr(self.total),
               N.dev_ptr(dice), N.dev_ptr(out), N.stream())
        self.counts, self.dice = counts, dice
        return out


_ACTIVATIONS = {'sigmoid': 0, 'softmax': 1}


def prob_onehot(logits, activation='sigmoid'):
    """Probabilities + one-hot argmax mask of [B,C,H,W] logits (inference_wrapper.py:17-24): sigmoid per channel (the
    reference) or softmax over the channels.  Binary logits with sigmoid take the two-class kernel."""
    if activation not in _ACTIVATIONS:
        raise ValueError(f"prob_onehot: activation must be 'sigmoid' or 'softmax', got {activation!r}")
    if logits.dim() != 4:
        raise ValueError('prob_onehot: [B,C,H,W] logits expected')
    if logits.shape[1] > 64:
        raise ValueError(f'prob_onehot: {logits.shape[1]} channels (at most 64 are supported)')
    x = _c(logits.float())
    prob, onehot = torch.empty_like(x), torch.empty_like(x)
    B, C, H, W = x.shape
    if C == 2 and activation == 'sigmoid':
        N.call('ssseg_prob_onehot', N.dev_ptr(x, 'logits'), B, H * W, N.dev_ptr(prob), N.dev_ptr(onehot), N.stream())
    else:
        _device_checked('prob_onehot', logits=x)
        N.call('ssseg_prob_onehot_mc', N.dev_ptr(x, 'logits'), B, C, H * W, _ACTIVATIONS[activation], N.dev_ptr(prob),
               N.dev_ptr(onehot), N.stream())
    return prob, onehot


# ------------------------------------------------------------------------------------------------
# Active-learning pool selection (csrc/active.hip; reference get_active_learning_partition.py)
# ------------------------------------------------------------------------------------------------
def uncertainty_scores(logits):
    """Per-image uncertainty of [B,C,...] logits -> float32 [B,3]: the means over the pixels of the softmax entropy
    (get_active_learning_partition.py:94-95), of the least confidence 1 - p1 and of the margin score 1 - (p1 - p2).
    The entropy is log Z - sum p (x - max x): 0, not NaN, on a saturated pixel.  One pass over the logits, bitwise
    reproducible, and an image scores the same bits alone and inside a batch.  No autograd: this is selection.
    Non-contiguous or non-fp32 logits are converted first."""
    if logits.dim() < 3:
        raise ValueError(f'uncertainty_scores: expected [B, C, ...] logits, got {tuple(logits.shape)}')
    B, C = logits.shape[:2]
    if not 2 <= C <= 64:
        raise ValueError(f'uncertainty_scores: {C} channels (the kernel covers 2 <= C <= 64)')
    if B < 1 or logits[0, 0].numel() < 1:
        raise ValueError(f'uncertainty_scores: empty logits {tuple(logits.shape)}')
    x = _c(logits.detach().float())
    HW = x[0, 0].numel()
    ptr = N.dev_ptr(x, 'logits')
    out = torch.empty((B, 3), device=x.device, dtype=torch.float32)
    nb = N.lib().ssseg_uncertainty_workspace_bytes(B, C, HW)
    ws = N.workspace(nb, x.device)
    N.call('ssseg_uncertainty_scores', ptr, B, C, HW, N.dev_ptr(out), N.dev_ptr(ws), nb, N.stream())
    return out


class KMeansResult(tuple):
    """(centroids [K,D] float64, labels [N] int32, inertia 0-d float64, n_iter 0-d int32, seed_idx [K] int32 or None),
    all on the device: reading one of them is the only synchronisation of a fit."""
    __slots__ = ()
    _fields = ('centroids', 'labels', 'inertia', 'n_iter', 'seed_idx')

    def __new__(cls, *vals):
        return tuple.__new__(cls, vals)

    centroids = property(lambda s: s[0])
    labels = property(lambda s: s[1])
    inertia = property(lambda s: s[2])
    n_iter = property(lambda s: s[3])
    seed_idx = property(lambda s: s[4])


def kmeans(X, k, *, u=None, init=None, tol=1e-6, max_iter=300):
    """Deterministic k-means of the rows of X [N,D] (fp32 on the device), 1 <= k <= min(64, N), in fp64.

    Exactly one of `u` (k uniforms in [0,1): k-means++ seeding, the scans in index order on the device) and `init`
    ([k,D] initial centroids).  Lloyd iterations: lowest centroid index on an exact tie, fp64 means in a fixed order,
    an empty cluster keeps its centroid; stops after max_iter iterations or once the summed squared centroid shift is
    <= tol * mean_d Var(X[:,d]) (sklearn's rule), decided on the device.  -> KMeansResult."""
    if (u is None) == (init is None):
        raise ValueError('kmeans: give exactly one of u (k-means++ uniforms) and init (initial centroids)')
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError('kmeans: X must be a [N,D] tensor')
    ptr = N.dev_ptr(X, 'X')
    n, d = X.shape
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError(f'kmeans: k = {k} (1 <= k <= 64 is supported)')
    if k > n:
        raise ValueError(f'kmeans: k = {k} clusters for {n} points')
    if d < 1:
        raise ValueError('kmeans: X has no columns')
    if not tol >= 0 or not 1 <= int(max_iter) <= 100000:
        raise ValueError(f'kmeans: tol = {tol!r}, max_iter = {max_iter!r}')
    X = _c(X.detach().float())
    ptr = N.dev_ptr(X, 'X')
    dev = X.device
    nb = N.lib().ssseg_kmeans_workspace_bytes(n, d, k)
    ws = N.workspace(nb, dev)
    labels = torch.empty(n, device=dev, dtype=torch.int32)
    inertia = torch.empty((), device=dev, dtype=torch.float64)
    n_iter = torch.empty((), device=dev, dtype=torch.int32)
    seed_idx = None
    if u is not None:
        u = torch.as_tensor(u, dtype=torch.float32).reshape(-1)
        if u.numel() != k:
            raise ValueError(f'kmeans: u must hold k = {k} uniforms, got {u.numel()}')
        if bool(((u < 0) | (u >= 1)).any()):
            raise ValueError('kmeans: u must lie in [0, 1)')
        u = _c(u.to(dev))
        cent = torch.empty((k, d), device=dev, dtype=torch.float64)
        seed_idx = torch.empty(k, device=dev, dtype=torch.int32)
        N.call('ssseg_kmeans_seed', ptr, n, d, k, N.dev_ptr(u), N.dev_ptr(seed_idx), N.dev_ptr(cent), N.dev_ptr(ws), nb,
               N.stream())
    else:
        init = torch.as_tensor(init)
        if tuple(init.shape) != (k, d):
            raise ValueError(f'kmeans: init must be [{k},{d}], got {tuple(init.shape)}')
        cent = init.detach().to(device=dev, dtype=torch.float64).contiguous().clone()
    N.call('ssseg_kmeans_fit', ptr, n, d, k, float(tol), int(max_iter), N.dev_ptr(cent), N.dev_ptr(labels),
           N.dev_ptr(inertia), N.dev_ptr(n_iter), N.dev_ptr(ws), nb, N.stream())
    return KMeansResult(cent, labels, inertia, n_iter, seed_idx)
