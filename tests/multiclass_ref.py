"""fp64 torch restatements of the multi-class kernels (csrc/multiclass.hip), for the tests of test_multiclass*.py.

* consistency_softmax: train.py:97-108 with the two commented softmax lines (:97, :99) in place of the sigmoid ones,
  plus the per-pixel weight w of the geometric consistency; its gradient comes from autograd.
* seg_metrics: train.py:171-175 with num_classes = C, metrics.dice_metric (metrics.py:1-7) and lovasz.iou
  (lovasz.py:54-73, per_image=False), from a dense mask or a label map with an ignore value.
* prob_onehot: models/inference_wrapper.py:17-24 for C classes with either activation.
"""
import numpy as np
import torch
import torch.nn.functional as F


def consistency_softmax(student, teacher, thr, w=None, activation='softmax'):
    """-> (loss, cm.mean(), cm.sum()); student / teacher [B,C,H,W] (any float dtype: computed in it), w [B,H,W]"""
    if activation == 'softmax':
        pt = torch.softmax(teacher, dim=1)
        ps = torch.softmax(student, dim=1)
    else:
        pt = torch.sigmoid(teacher)
        ps = torch.sigmoid(student)
    # the decision is the kernel's fp32 one where the inputs are fp32 values held in fp64: the tests keep every
    # pixel's max pt at least 1e-3 away from thr, so both precisions decide alike
    cm = (pt.max(dim=1).values > thr).to(pt)
    if w is not None:
        cm = cm * w.to(pt)
    loss = torch.pow(ps - pt, exponent=2.0)
    loss = (loss.sum(dim=1) * cm).sum() / cm.sum()
    return loss.mean(), cm.mean(), cm.sum()


def consistency_softmax_grad(student, teacher, thr, w=None, gout=1.0, activation='softmax'):
    """fp64 loss, cm mean, cm sum and d (gout * loss) / d student as numpy"""
    s = student.detach().double().requires_grad_(True)
    t = teacher.detach().double()
    loss, cm, cnt = consistency_softmax(s, t, thr, None if w is None else w.double(), activation)
    (loss * gout).backward()
    return loss.detach().numpy(), cm.numpy(), cnt.numpy(), s.grad.numpy()


def iou(pred, label, C, ignore=None):
    """lovasz.iou (lovasz.py:54-73) with per_image=False, EMPTY=1, as fractions in fp64 (the reference returns
    100 * these); pred, label: integer tensors of one shape"""
    out = []
    for i in range(C):
        inter = ((label == i) & (pred == i)).sum()
        union = ((label == i) | ((pred == i) & (label != (ignore if ignore is not None else -1)))).sum()
        out.append(float(inter) / float(union) if union else 1.0)
    return np.array(out, np.float64)


def confusion(pred, label, C, ignore=None):
    """[C,C] int64: rows label, columns prediction, the ignored pixels left out"""
    keep = torch.ones_like(label, dtype=torch.bool) if ignore is None else label != ignore
    idx = label[keep].long() * C + pred[keep].long()
    return torch.bincount(idx, minlength=C * C).view(C, C)


def predictions(logits, size):
    """train.py:171-172: argmax -> one-hot -> nearest resize to `size`; -> ([B,C,H,W] one-hot fp64, [B,H,W] ids)"""
    C = logits.shape[1]
    one_hot = F.one_hot(torch.argmax(logits, dim=1), num_classes=C).permute(0, 3, 1, 2).double()
    one_hot = F.interpolate(one_hot, size=tuple(size), mode='nearest')
    return one_hot, one_hot.argmax(dim=1)


def seg_metrics(logits, target, ignore=None, total=None):
    """One SegMetricsMC.update: logits [B,C,h,w], target a dense mask [B,C,H,W] or an int64 label map [B,H,W].
    -> dict(conf [C,C] int64, dice [B,2] int64, dice_mean, ious [C] fractions, miou) with the IoUs over total + conf
    where a running matrix `total` is given."""
    logits = logits.detach().cpu()
    target = target.detach().cpu()
    B, C = logits.shape[:2]
    pred_1h, pred = predictions(logits, target.shape[-2:])
    if target.dim() == 3:
        keep = (target != ignore) if ignore is not None else torch.ones_like(target, dtype=torch.bool)
        label = target
        t_1h = F.one_hot(torch.where(keep, target, torch.zeros_like(target)), C).permute(0, 3, 1, 2).double()
        t_1h = t_1h * keep.unsqueeze(1)
        pred_1h = pred_1h * keep.unsqueeze(1)
    else:
        label = torch.argmax(target, dim=1)
        t_1h = (target > 0.5).double()           # train.py:173
    # metrics.dice_metric(pred[:, 1:], t[:, 1:]) (metrics.py:1-7, train.py:175)
    inter = (pred_1h[:, 1:] * t_1h[:, 1:]).sum(dim=(1, 2, 3))
    card = (pred_1h[:, 1:] + t_1h[:, 1:]).sum(dim=(1, 2, 3))
    dice = (2. * inter + 1.) / (card + 1.)
    conf = confusion(pred, label, C, ignore if target.dim() == 3 else None)
    run = conf if total is None else total + conf
    i = run.diagonal().double()
    u = run.sum(0).double() + run.sum(1).double() - i
    ious = torch.where(u > 0, i / u.clamp(min=1), torch.ones_like(i)).numpy()
    return dict(conf=conf, dice=torch.stack([inter, card], 1).round().long(), dice_mean=float(dice.mean()),
                ious=ious, miou=float(ious.mean()))


def prob_onehot(logits, activation='sigmoid'):
    """-> (fp64 probabilities, fp32 one-hot of the argmax), both [B,C,H,W]"""
    x = logits.detach().cpu().double()
    prob = torch.sigmoid(x) if activation == 'sigmoid' else torch.softmax(x, dim=1)
    onehot = F.one_hot(torch.argmax(logits.detach().cpu(), dim=1), logits.shape[1]).permute(0, 3, 1, 2).float()
    return prob, onehot


def confident_teacher(shape, thr, seed, frac=0.6, margin=1e-3, scale=1.0):
    """Teacher logits [B,C,H,W] (fp32) whose per-pixel softmax maximum is above thr + margin on a designed set of
    pixels and below thr - margin on the rest; -> (logits, confident [B,H,W] bool).  A confident pixel gets one class
    lifted far above the others; an unconfident one gets its two largest logits made equal (max p <= 1/2 < thr), or,
    for C == 1 (softmax == 1 everywhere), stays as it is: every pixel is confident."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, C, H, W, generator=g)
    conf = torch.rand(B, H, W, generator=g) < frac
    if C == 1:
        return t * scale, torch.ones(B, H, W, dtype=torch.bool)
    top = torch.randint(0, C, (B, H, W), generator=g)
    lift = F.one_hot(top, C).permute(0, 3, 1, 2).bool()
    # confident: the lifted class leads by >= 4 + log(C): p_max >= 1 / (1 + (C-1) e^-lead) > 0.98
    lead = t.amax(dim=1, keepdim=True) + 4.0 + float(np.log(C))
    t_conf = torch.where(lift, lead.expand_as(t), t)
    # unconfident: the runner-up is raised to the maximum (an exact tie: max p <= 1/2)
    second = F.one_hot((top + 1) % C, C).permute(0, 3, 1, 2).bool()
    mx = torch.maximum(t.amax(dim=1, keepdim=True), torch.zeros(()))
    t_unc = torch.where(lift | second, mx.expand_as(t), t)
    t = torch.where(conf.unsqueeze(1), t_conf, t_unc) * scale
    return t.contiguous(), conf
