"""fp64 torch restatement of the pseudo-label consistency loss (ssseg_consistency_ce_fwd / _bwd, csrc/multiclass.hip),
for test_pseudo_ce*.py: cross-entropy of the student against the teacher's hard label, weighted by the teacher's
confidence (FixMatch: Sohn et al. 2020, eq. 4; ClassMix: Olsson et al. 2021, section 3.2).  Built on torch.argmax,
F.cross_entropy(reduction='none') and torch.where; the gradient comes from autograd.
"""
import torch
import torch.nn.functional as F


def pseudo_ce(student, teacher, thr, w=None, weighting='pixel'):
    """-> (loss, sum(w cm) / npix, sum(w cm), sum(w)); student / teacher [B,C,H,W] (any float dtype: computed in it),
    w [B,H,W].  The teacher is a constant."""
    teacher = teacher.detach()
    y = torch.argmax(teacher, dim=1)
    # the decision is the kernel's fp32 one where the inputs are fp32 values held in fp64: the tests keep every
    # pixel's max pt at least 1e-3 away from thr, so both precisions decide alike
    conf = torch.softmax(teacher, dim=1).max(dim=1).values
    cm = conf > thr
    ce = F.cross_entropy(student, y, reduction='none')
    wt = torch.ones_like(ce) if w is None else w.to(ce)
    n_w = wt.sum()
    s_cm = torch.where(cm, wt, torch.zeros_like(wt)).sum()
    if weighting == 'pixel':
        # selected, not multiplied: an unconfident pixel adds exactly 0 whatever its cross-entropy
        loss = torch.where(cm, wt * ce, torch.zeros_like(ce)).sum() / n_w
    elif weighting == 'batch':
        loss = (s_cm / n_w) * ((wt * ce).sum() / n_w)
    else:
        raise ValueError(weighting)
    return loss, s_cm / cm.numel(), s_cm, n_w


def pseudo_ce_grad(student, teacher, thr, w=None, weighting='pixel', gout=1.0):
    """fp64 loss, cm mean, sum(w cm) and d (gout * loss) / d student as numpy"""
    s = student.detach().double().requires_grad_(True)
    t = teacher.detach().double()
    loss, cm, s_cm, _ = pseudo_ce(s, t, thr, None if w is None else w.double(), weighting)
    (loss * gout).backward()
    return loss.detach().numpy(), cm.numpy(), s_cm.numpy(), s.grad.numpy()


def pseudo_ce_loop(student, teacher, thr, w=None, weighting='pixel'):
    """the same loss written out pixel by pixel in Python floats (math.exp / math.log, no torch reduction)"""
    import math
    B, C, H, W = student.shape
    n_w = s_cm = s_conf = s_all = 0.0
    for b in range(B):
        for i in range(H):
            for j in range(W):
                t = [float(v) for v in teacher[b, :, i, j]]
                s = [float(v) for v in student[b, :, i, j]]
                y, mt = 0, t[0]
                for c in range(1, C):
                    if t[c] > mt:
                        y, mt = c, t[c]
                conf = 1.0 / sum(math.exp(v - mt) for v in t)
                ms = max(s)
                ce = math.log(sum(math.exp(v - ms) for v in s)) + ms - s[y]
                wv = 1.0 if w is None else float(w[b, i, j])
                n_w += wv
                s_all += wv * ce
                if conf > thr:
                    s_cm += wv
                    s_conf += wv * ce
    loss = s_conf / n_w if weighting == 'pixel' else (s_cm / n_w) * (s_all / n_w)
    return loss, s_cm / (B * H * W), s_cm, n_w
