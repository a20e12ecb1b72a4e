"""Reversible augmentations — drop-in for reference reversible_augmentations.py (Rotate :5-23, Rescale :26-49),
which wraps kornia.rotate / kornia.resize and is imported (never called) by train.py:5.

Same API and sampling: Rotate(max_angle) draws one angle ~ U(-|max_angle|, |max_angle|) per apply() from the
CPU generator and applies it to every tensor of the list; reverse() rotates back by -angle.  Rescale(min, max)
draws one scale per apply() and resizes to (int(H*s), int(W*s)); reverse() resizes by 1/s.  Compute runs on the
device kernels: ssseg_rotate_fwd/bwd (bilinear about the centre, zero padding, differentiable) and the bilinear
interpolation kernel (align_corners=False, kornia.resize's default).  kornia is absent here and unpinned by the
reference, so parity with kornia itself is unpinned; the kernels are checked against a torch grid_sample
restatement (tests/test_hip_losses.py).

RotateRescale (not in the reference; its trainer's stated plan, train.py:16-17) is both as one per-sample affine warp
at a fixed size, which a batch and a captured step can carry: the consistency branch's student view."""
import torch

from ssseg import ops


class Rotate:
    def __init__(self, max_angle):
        self.max_angle = torch.abs(torch.tensor([max_angle], dtype=torch.float32))
        self.distribution = torch.distributions.uniform.Uniform(low=-self.max_angle, high=self.max_angle)
        self.angle = None

    def apply(self, inputs):
        self.angle = self.distribution.sample()
        return [ops.rotate(t, float(self.angle)) for t in inputs]

    def reverse(self, inputs):
        return [ops.rotate(t, -float(self.angle)) for t in inputs]


class Rescale:
    def __init__(self, min_scale, max_scale):
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.distribution = torch.distributions.uniform.Uniform(low=torch.tensor([min_scale], dtype=torch.float32),
                                                                high=torch.tensor([max_scale], dtype=torch.float32))
        self.scale = None

    def apply(self, inputs):
        self.scale = self.distribution.sample().item()
        return [ops.interpolate_bilinear(t, (int(t.size(2) * self.scale), int(t.size(3) * self.scale)))
                for t in inputs]

    def reverse(self, inputs):
        return [ops.interpolate_bilinear(t, (int(t.size(2) * (1. / self.scale)), int(t.size(3) * (1. / self.scale))))
                for t in inputs]


class RotateRescale:
    """Rotate and Rescale as ONE per-sample affine warp at a fixed size (what a batch and a captured step can carry):
    apply() draws theta_b ~ U(-max_angle, max_angle) and s_b ~ U(min_scale, max_scale) per sample -- the two
    distributions above -- and warps every tensor of the list with A(theta_b, s_b) (ssseg_affine_warp_fwd; the content
    turns counter-clockwise by theta and is magnified by s about the centre); reverse() warps with the inverse and
    keeps that call's validity map ([B, H, W], 1 where the pixel came from inside the frame) in .valid.

    source='device' (default): Philox draws on CowMix's per-device counter and seed (ssseg_affine_draw_dev), no host
    sync, and a captured step replays fresh views.  source='cpu': B angles, then B scales, from the CPU torch
    generator (parity tests).  set_params(angles, scales) fixes the parameters outright (nothing is drawn)."""

    def __init__(self, max_angle, min_scale, max_scale, source='device'):
        max_angle, min_scale, max_scale = float(max_angle), float(min_scale), float(max_scale)
        if not 0.0 <= max_angle <= 180.0:
            raise ValueError(f'RotateRescale: max_angle {max_angle} outside [0, 180]')
        # the backward's gather box is (|ia| + |ib| + 1)^2-bounded: at most 13 x 13 for scales within [1/4, 4]
        if not 0.25 <= min_scale <= max_scale <= 4.0:
            raise ValueError(f'RotateRescale: scales ({min_scale}, {max_scale}) outside 0.25 <= min <= max <= 4')
        if source not in ('device', 'cpu'):
            raise ValueError(f"RotateRescale: source {source!r} is neither 'device' nor 'cpu'")
        self.max_angle, self.min_scale, self.max_scale, self.source = max_angle, min_scale, max_scale, source
        self.fixed = None
        self.mats = self.mats_inv = self.valid = None

    def set_params(self, angles, scales):
        angles = torch.as_tensor(angles, dtype=torch.float64).reshape(-1)
        scales = torch.as_tensor(scales, dtype=torch.float64).reshape(-1)
        if angles.numel() != scales.numel():
            raise ValueError('RotateRescale.set_params: one angle and one scale per sample')
        if float(angles.abs().max()) > 180.0 or float(scales.min()) < 0.25 or float(scales.max()) > 4.0:
            raise ValueError('RotateRescale.set_params: angles outside [-180, 180] or scales outside [0.25, 4]')
        self.fixed = (angles, scales)

    def _draw(self, example):
        B, _, H, W = example.shape
        dev = example.device
        if self.fixed is not None:
            if self.fixed[0].numel() != B:
                raise ValueError(f'RotateRescale: {self.fixed[0].numel()} fixed parameters for a batch of {B}')
            return ops.affine_mats(self.fixed[0], self.fixed[1], H, W, dev)
        if self.source == 'cpu':
            angles = (torch.rand(B, dtype=torch.float32) * 2 - 1) * self.max_angle
            scales = self.min_scale + torch.rand(B, dtype=torch.float32) * (self.max_scale - self.min_scale)
            return ops.affine_mats(angles, scales, H, W, dev)
        import cowmix
        from ssseg import native as N
        mats = torch.empty(B, 6, device=dev)
        inv = torch.empty(B, 6, device=dev)
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        ctr = cowmix._DEVICE_RNG['ctr'].get(key)
        if ctr is None:
            ctr = cowmix._DEVICE_RNG['ctr'][key] = torch.zeros(1, dtype=torch.int64, device=dev)
        N.call('ssseg_affine_draw_dev', N.dev_ptr(mats), N.dev_ptr(inv), B, H, W, self.max_angle, self.min_scale,
               self.max_scale, cowmix._device_seed(dev), N.dev_ptr(ctr), N.stream())
        return mats, inv

    def apply(self, inputs):
        with torch.no_grad():
            self.mats, self.mats_inv = self._draw(inputs[0])
        return [ops.affine_warp(t, self.mats, self.mats_inv) for t in inputs]

    def reverse(self, inputs):
        out = []
        for k, t in enumerate(inputs):
            if k == 0:
                y, self.valid = ops.affine_warp(t, self.mats_inv, self.mats, want_valid=True)
            else:
                y = ops.affine_warp(t, self.mats_inv, self.mats)
            out.append(y)
        return out
