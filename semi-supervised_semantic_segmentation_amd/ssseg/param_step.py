"""The tail of a training step as ONE launch (ssseg_param_step, csrc/param_step.hip): clip + SGD, teacher EMA, the
bf16 repack of every conv weight of student and teacher, and the gradient clear -- instead of ssseg_sgd_step,
ssseg_ema_update, two ssseg_weight_pack_batch launches and the gradient memset, which read the parameters three times.

group() turns the arena layout and the packs of its conv weights into the kernel's descriptor table (pure Python, no
device); plan_for() decides whether a (student, teacher, optimizer) triple can take the fused launch and caches the
device tables on the student, like nn.invalidate_packed caches the pack tables.  Whoever cannot take it runs the
separate sequence unchanged.  SSSEG_PARAM_STEP=0 disables the fused launch (A/B runs).
"""
import os

import torch

from . import native as N
from . import nn as snn
from . import ops

SGD, EMA, CLEAR = 1, 2, 4
MAX_TAPS = 135
DESC_WORDS, PACK_WORDS = 10, 11


def enabled():
    return os.environ.get('SSSEG_PARAM_STEP', '1') != '0'


def group(numel, weights):
    """Descriptor rows of ssseg_param_step for an arena of `numel` elements.

    weights: (offset, (A, B, Rs, Ss), packs) per conv weight that has packs, packs = (dst_ptr, teacher, spec) with
    spec the ssseg_weight_pack arguments (Kd, Kr, Cd, Rs, Ss, Cp, layout, r0, rstep, Rn, s0, sstep, Sn).  Returns
    (desc_rows, pack_rows): one conv descriptor per weight -- however many packs and layouts it has, so each weight is
    updated once -- and one flat range per gap between them, together covering [0, numel) exactly once."""
    if numel % 4:
        raise ValueError('param_step.group: the arena length must be a multiple of 4 elements')
    descs, packs, pos = [], [], 0
    for off, (A, B, Rs, Ss), plist in sorted(weights, key=lambda w: w[0]):
        n = A * B * Rs * Ss
        if off % 4 or off < pos or off + n > numel:
            raise ValueError(f'param_step.group: weight at {off} (+{n}) overlaps its neighbour, leaves the arena or '
                             'is not 16-byte aligned')
        if not 1 <= Rs * Ss <= MAX_TAPS or n < 1 or n >= 2 ** 31 or not plist:
            raise ValueError(f'param_step.group: weight at {off}: {Rs}x{Ss} taps, {n} elements, {len(plist)} packs')
        if off > pos:
            descs.append((pos, off - pos, 0, 0, 0, 0, 0, 0, 0, 0))
        Ap, Bp = A, B
        p0 = len(packs)
        for dst, teacher, (Kd, Kr, Cd, rs, ss, Cp, layout, r0, rstep, Rn, s0, sstep, Sn) in plist:
            if layout not in (0, 1) or (rs, ss) != (Rs, Ss) or (Kr, Cd) != ((A, B) if layout == 0 else (B, A)):
                raise ValueError(f'param_step.group: weight at {off}: pack spec does not describe a [{A}][{B}][{Rs}]'
                                 f'[{Ss}] source')
            taps_ok = all(n >= 0 and (n == 0 or (0 <= t0 < lim and 0 <= t0 + (n - 1) * st < lim))
                          for t0, st, n, lim in ((r0, rstep, Rn, Rs), (s0, sstep, Sn, Ss)))
            if Kd < Kr or Cp < Cd or Kd * Rn * Sn * Cp >= 2 ** 31 or not taps_ok:
                raise ValueError(f'param_step.group: weight at {off}: bad pack extents')
            Ap = max(Ap, Kd if layout == 0 else Cp)
            Bp = max(Bp, Cp if layout == 0 else Kd)
            packs.append((dst, int(bool(teacher)), layout, Kd, Cp, r0, rstep, Rn, s0, sstep, Sn))
        descs.append((off, n, A, B, Rs, Ss, Ap, Bp, p0, len(packs) - p0))
        pos = off + n
    if pos < numel:
        descs.append((pos, numel - pos, 0, 0, 0, 0, 0, 0, 0, 0))
    return descs, packs


def _conv_rows(model, arena, teacher, reasons):
    """(offset, dims, packs) of every conv of `model` that has packs; None (with a reason) when one of them cannot be
    served by the fused launch."""
    rows = []
    base = arena.data.data_ptr()
    for m in model.modules():
        if not isinstance(m, snn._ConvBase) or not m._ssseg_packs:
            continue
        w = m.weight
        if getattr(w, '_ssseg_arena', None) is not arena or not w.is_contiguous() or w.dim() != 4:
            reasons.append('a packed conv weight outside the arena')
            return None
        if w.shape[2] * w.shape[3] > MAX_TAPS:
            reasons.append('a filter of more than 135 taps')
            return None
        plist = []
        for key, t in m._ssseg_packs.items():
            if key[1] != torch.bfloat16:
                reasons.append('a pack that is not bf16')
                return None
            plist.append((t.data_ptr(), teacher, m._ssseg_specs[key]))
        rows.append(((w.data_ptr() - base) // 4, tuple(w.shape), plist))
    return rows


def eligible(student_arena, teacher_arena, optimizer, reasons=None):
    """The rule of the fused path, without the packs: one fp32 arena per model of the same layout, plain SGD over
    the student's arena, no loss scaler."""
    from . import optim
    reasons = reasons if reasons is not None else []
    if not enabled():
        reasons.append('SSSEG_PARAM_STEP=0')
    elif type(optimizer) is not optim.SGD:
        reasons.append('not plain SGD')
    elif optimizer.grad_scaler is not None:
        reasons.append('loss-scaled gradients')
    elif student_arena is None or teacher_arena is None or optimizer.arena is not student_arena:
        reasons.append('no flat arena per model')
    elif student_arena.grad is None or not student_arena.data.is_cuda or student_arena.numel % 4:
        reasons.append('arena without gradients or not on the device')
    elif student_arena.data.dtype != torch.float32 or teacher_arena.data.dtype != torch.float32:
        reasons.append('arena not fp32')
    elif not student_arena.compatible(teacher_arena) or teacher_arena.data.device != student_arena.data.device:
        reasons.append('student and teacher arenas differ')
    return not reasons


def plan_for(student, teacher, optimizer):
    """The cached fused-step plan (device tables) of this triple, or None where the separate sequence must run.  The
    tables are rebuilt when a conv gains or drops a pack or an arena moves; never inside a graph capture, where a
    stale plan means the separate sequence."""
    sa, ta = getattr(student, '_ssseg_arena', None), getattr(teacher, '_ssseg_arena', None)
    if not eligible(sa, ta, optimizer):
        return None
    sig = (snn._PACK_EPOCH[0], id(teacher), id(optimizer), sa.data.data_ptr(), ta.data.data_ptr())
    cache = student.__dict__.get('_ssseg_param_step')
    if cache is not None and cache[0] == sig:
        return cache[1]
    if torch.cuda.is_current_stream_capturing():
        return None
    plan = None
    reasons = []
    srows = _conv_rows(student, sa, 0, reasons)
    trows = _conv_rows(teacher, ta, 1, reasons) if srows is not None else None
    # "pack tables built": both models have been through nn.invalidate_packed with this set of packs
    built = all(m.__dict__.get('_ssseg_pack_fast', (None,))[0] == snn._PACK_EPOCH[0] for m in (student, teacher))
    if srows is not None and trows is not None and built and (srows or trows):
        merged = {}
        for off, dims, plist in srows + trows:
            ent = merged.setdefault(off, (dims, []))
            if ent[0] != dims:
                ent = None
                break
            ent[1].extend(plist)
        else:
            descs, packs = group(sa.numel, [(off, dims, pl) for off, (dims, pl) in merged.items()])
            dev = sa.data.device
            plan = (torch.tensor(descs, dtype=torch.int64).to(dev), len(descs),
                    torch.tensor(packs, dtype=torch.int64).to(dev))
    if plan is not None or srows is None or trows is None or built:   # (tables not built yet: look again next step)
        student.__dict__['_ssseg_param_step'] = (sig, plan)
    return plan


def launch(plan, param, grad, buf, ema, lr, momentum, wd, max_norm, sqnorm, first, alpha, flags, amp_state=None):
    descs, n, packs = plan
    N.call('ssseg_param_step', N.dev_ptr(param, 'param'), N.dev_ptr(grad), N.dev_ptr(buf), N.dev_ptr(ema),
           N.dev_ptr(snn._graph_ref(descs)), n, N.dev_ptr(snn._graph_ref(packs)), float(lr), float(momentum), float(wd),
           float(max_norm), N.dev_ptr(sqnorm), int(bool(first)), N.dev_ptr(amp_state), float(alpha), int(flags),
           N.stream())


def step(plan, optimizer, teacher_arena, max_norm, alpha, sgd=True):
    """The fused launch for optimizer (ssseg.optim.SGD) and the teacher's arena: with sgd, clip + SGD + EMA + repack +
    gradient clear (the next arena.zero_grad() is then a no-op); without, the EMA and the teacher's repack alone (a
    step that takes no optimizer step: gradient accumulation, the reference's step 0)."""
    a = optimizer.arena
    g = optimizer.param_groups[0]
    max_norm = max_norm or 0.0
    if sgd and max_norm > 0:
        N.call('ssseg_zero', N.dev_ptr(optimizer._sq), 4, N.stream())
        ops.sqnorm_(a.grad, optimizer._sq)
    launch(plan, a.data, a.grad, optimizer.buf, teacher_arena.data, g['lr'], g['momentum'] if optimizer.buf is not None
           else 0.0, g['weight_decay'], max_norm, optimizer._sq if max_norm > 0 else None, optimizer._first, alpha,
           (SGD | CLEAR | EMA) if sgd else EMA)
    if sgd:
        optimizer._first = False
        a.cleared = True
