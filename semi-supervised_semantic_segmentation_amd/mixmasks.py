"""ClassMix and CutMix masks for the consistency branch, next to CowMix (cowmix.py) -- build-defined: the reference
mixes with CowMix only.  Both return B x 1 x H x W masks in {0, 1} for cowmix.mix_with_mask.

ClassMix (Olsson et al. 2021): the mask follows the teacher's own prediction on batch A -- per image, half of the
classes its argmax map holds (ceil(n/2) of n, chosen uniformly at random) -- so objects are cut along their predicted
borders.  CutMix (French et al. 2020): one random box per image whose area is the proportion p of the image.

Random inputs (a 31-bit key per image and class, whose order picks the classes; four uniforms per image) come from:
  DRAW_SOURCE = 'device' (default): Philox on CowMix's per-device seed and counter (ssseg_mixmask_draw_dev), no host
      sync; a captured step replays fresh masks.  A call advances the counter by B * (ceil(C/4) + 1) (CutMix: C = 1).
  DRAW_SOURCE = 'host': the CPU torch generator, torch.randint(0, 2**31, (B, C)) / torch.rand(B, 4); the parity tests.
set_draws(keys=, params=) fixes the draws outright (like RotateRescale.set_params) until it is called without them.
"""
import torch

import cowmix
from ssseg import native as N
from ssseg import ops

MIX_MASKS = ('cowmix', 'cutmix', 'classmix')
DRAW_SOURCE = 'device'
_FIXED = {'keys': None, 'params': None}


def mix_mask_kind(tc):
    """config['train']['mix_mask']: 'cowmix' (the reference, and the default), 'cutmix' or 'classmix'."""
    kind = tc.get('mix_mask', 'cowmix')
    if kind not in MIX_MASKS:
        raise ValueError(f"mix_mask must be one of {MIX_MASKS}, got {kind!r}")
    return kind


def set_draws(keys=None, params=None):
    """Fix the ClassMix keys [B,C] (integers in [0, 2^31)) and / or the CutMix params [B,4] (in [0,1)) of every following
    call; None returns that draw to DRAW_SOURCE."""
    if keys is not None:
        keys = torch.as_tensor(keys).to(torch.int64)
        if keys.dim() != 2 or bool((keys < 0).any()) or bool((keys >= 2 ** 31).any()):
            raise ValueError('set_draws: keys must be [B,C] integers in [0, 2^31)')
        keys = keys.to(torch.int32)
    if params is not None:
        params = torch.as_tensor(params, dtype=torch.float32)
        if params.dim() != 2 or params.shape[1] != 4 or bool((params < 0).any()) or bool((params >= 1).any()):
            raise ValueError('set_draws: params must be [B,4] in [0,1)')
    _FIXED['keys'], _FIXED['params'] = keys, params


def draws_fixed():
    return _FIXED['keys'] is not None or _FIXED['params'] is not None


def capturable(kind):
    """Whether a captured step replays fresh masks of this kind: the draws come from the device counter."""
    return kind == 'cowmix' or (DRAW_SOURCE == 'device' and not draws_fixed())


def counter_advance(B, C):
    """What one device draw adds to the Philox counter."""
    return B * ((C + 3) // 4 + 1)


def draw(which, B, C, dev):
    """The 'keys' [B,C] int32 or the 'params' [B,4] f32 of one call on `dev`: fixed, from the host generator, or from the
    device counter (which a call advances by counter_advance(B, C))."""
    fixed = _FIXED[which]
    shape = (B, C) if which == 'keys' else (B, 4)
    if fixed is not None:
        if tuple(fixed.shape) != shape:
            raise ValueError(f'mixmasks: fixed {which} of shape {tuple(fixed.shape)} for a call that needs {shape}')
        return fixed.to(dev)
    if DRAW_SOURCE == 'host':
        return (torch.randint(0, 2 ** 31, shape).to(torch.int32) if which == 'keys' else torch.rand(*shape)).to(dev)
    if DRAW_SOURCE != 'device':
        raise ValueError(f"mixmasks.DRAW_SOURCE {DRAW_SOURCE!r} is neither 'device' nor 'host'")
    out = torch.empty(shape, device=dev, dtype=torch.int32 if which == 'keys' else torch.float32)
    seed = cowmix._device_seed(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ctr = cowmix._DEVICE_RNG['ctr'].get(key)
    if ctr is None:
        ctr = cowmix._DEVICE_RNG['ctr'][key] = torch.zeros(1, dtype=torch.int64, device=dev)
    N.call('ssseg_mixmask_draw_dev', N.dev_ptr(out) if which == 'keys' else None,
           N.dev_ptr(out) if which == 'params' else None, B, C, seed, N.dev_ptr(ctr), N.stream())
    return out


def generate_classmix_masks_like(teacher_logits_a):
    """B x 1 x H x W ClassMix masks of the teacher's logits on batch A [B,C,H,W], same dtype / device."""
    with torch.no_grad():
        B, C = teacher_logits_a.shape[:2]
        keys = draw('keys', B, C, teacher_logits_a.device)
        mask = ops.classmix_mask(teacher_logits_a, keys)
        if mask.dtype != teacher_logits_a.dtype:
            mask = mask.to(teacher_logits_a.dtype)
        return mask


def generate_cutmix_masks_like(example, mask_proportion_range):
    """B x 1 x H x W CutMix masks for the example batch [B,_,H,W], same dtype / device."""
    with torch.no_grad():
        B, _, H, W = example.shape
        params = draw('params', B, 1, example.device)
        mask = ops.cutmix_mask(params, H, W, mask_proportion_range)
        if mask.dtype != example.dtype:
            mask = mask.to(example.dtype)
        return mask
