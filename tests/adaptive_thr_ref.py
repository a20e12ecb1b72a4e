"""fp64 torch restatement of the self-adaptive per-class confidence thresholds (ssseg_adaptive_thr_update,
csrc/adaptive_thr.hip; FreeMatch: Wang et al., ICLR 2023, section 3.2, eqs. 5-8) and of the pseudo-label cross-entropy
with one threshold per class (ssseg_consistency_ce_cls_fwd / _bwd), for test_adaptive_thr*.py.

The rule, with the operation order that the device follows for thr:
    p = softmax(t) per pixel,  m = mean_pix max_c p,  q_c = mean_pix p_c           (all B H W pixels, sum / count)
    tau <- lam tau + (1 - lam) m,  ptilde_c <- lam ptilde_c + (1 - lam) q_c        (tau = ptilde_c = 1 / C at the start)
    thr_c = float32((ptilde_c / max_k ptilde_k) * tau)                             (fp64 operations, one rounding)
"""
import math

import torch

import pseudo_ce_ref as P


def sat_init(C):
    return {'tau': torch.tensor(1.0 / C, dtype=torch.float64),
            'ptilde': torch.full((C,), 1.0 / C, dtype=torch.float64), 'steps': 0}


def batch_stats(teacher):
    """-> (m, q[C]) in fp64: sums over all pixels divided by their count"""
    p = torch.softmax(teacher.detach().double(), dim=1)
    n = float(p.shape[0] * p[0, 0].numel())
    return p.amax(dim=1).sum() / n, p.sum(dim=tuple(d for d in range(p.dim()) if d != 1)) / n


def thresholds(state):
    pt = state['ptilde']
    return ((pt / pt.max()) * state['tau']).float()


def sat_update(state, teacher, momentum):
    """one update in place; -> (thr_c float32 [C], m, q)"""
    lam = float(momentum)
    m, q = batch_stats(teacher)
    state['tau'] = lam * state['tau'] + (1.0 - lam) * m
    state['ptilde'] = lam * state['ptilde'] + (1.0 - lam) * q
    state['steps'] += 1
    return thresholds(state), m, q


def sat_update_loop(tau, ptilde, teacher, momentum):
    """the same update written out pixel by pixel in Python floats; -> (tau, ptilde list, thr list of Python floats)"""
    B, C, H, W = teacher.shape
    sm, sq = 0.0, [0.0] * C
    for b in range(B):
        for i in range(H):
            for j in range(W):
                t = [float(v) for v in teacher[b, :, i, j]]
                mx = max(t)
                e = [math.exp(v - mx) for v in t]
                z = sum(e)
                sm += max(e) / z
                for c in range(C):
                    sq[c] += e[c] / z
    n = float(B * H * W)
    lam = float(momentum)
    tau = lam * tau + (1.0 - lam) * (sm / n)
    ptilde = [lam * ptilde[c] + (1.0 - lam) * (sq[c] / n) for c in range(C)]
    return tau, ptilde, [(v / max(ptilde)) * tau for v in ptilde]


def confidence(teacher):
    """fp64 max_c softmax(t) and the label torch.argmax gives, [B,H,W] each"""
    t = teacher.detach().double()
    return torch.softmax(t, dim=1).amax(dim=1), torch.argmax(t, dim=1)


def pseudo_ce(student, teacher, thr_c, w=None, weighting='pixel', label=None):
    """pseudo_ce_ref.pseudo_ce with the threshold thr_c[y] at the teacher's label y = torch.argmax(teacher) (`label`
    overrides where the threshold is read: the tests' mutated copies).  -> (loss, sum(w cm) / npix, sum(w cm), sum(w))"""
    y = torch.argmax(teacher.detach(), dim=1) if label is None else label
    return P.pseudo_ce(student, teacher, thr_c.to(student.dtype)[y], w, weighting)


def pseudo_ce_grad(student, teacher, thr_c, w=None, weighting='pixel', gout=1.0, label=None):
    """fp64 loss, cm mean, sum(w cm) and d (gout * loss) / d student as numpy (the gradient from autograd)"""
    s = student.detach().double().requires_grad_(True)
    loss, cm, s_cm, _ = pseudo_ce(s, teacher.detach().double(), thr_c.double(), None if w is None else w.double(),
                                  weighting, label)
    (loss * gout).backward()
    return loss.detach().numpy(), cm.numpy(), s_cm.numpy(), s.grad.numpy()


def min_distance(teacher, thr_c):
    """the smallest distance of any pixel's fp64 confidence from its own threshold thr_c[y]"""
    conf, y = confidence(teacher)
    return float((conf - thr_c.double()[y]).abs().min())


def confident(teacher, thr_c):
    conf, y = confidence(teacher)
    return conf > thr_c.double()[y]


TIERS = (0.4, 0.3, 0.3)
# tiered_teacher seeds TIER_SEED, + 1, + 2 at (2, C, 17, 31), C in 2, 3, 5, 19: over three consecutive updates with
# momentum 0 and 0.5 every pixel's confidence stays at least 7e-3 from its own threshold (the tests assert 1e-3 before
# they compare masks: a condition on the inputs; many seeds put the 0.75 tier closer to one class's threshold)
TIER_SEED = 379


def tiered_teacher(shape, seed):
    """fp32 teacher logits [B,C,H,W] with three kinds of pixel.  Every pixel has a class y drawn with weight c + 1 and
    an offset a ~ N(0, 1) common to its channels; 40 % have t_y = a + log(99 (C - 1)) (confidence 0.99), 30 % have
    t_y = a + log(3 (C - 1)) (0.75), 30 % have t_y = t_(y + 1) % C = a + 30, an exact two-way tie (0.5) that the
    first-maximum rule has to place.  C = 1 has its one logit a."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, H, W, generator=g)
    t = a.unsqueeze(1).repeat(1, C, 1, 1)
    if C == 1:
        return t.contiguous()
    y = torch.multinomial(torch.arange(1, C + 1, dtype=torch.float64), B * H * W, replacement=True,
                          generator=g).view(B, 1, H, W)
    u = torch.rand(B, H, W, generator=g)
    tier = (u >= TIERS[0]).long() + (u >= TIERS[0] + TIERS[1]).long()
    lift = torch.tensor([math.log(99.0 * (C - 1)), math.log(3.0 * (C - 1)), 30.0])[tier]
    t.scatter_(1, y, (a + lift).unsqueeze(1))
    tie = (tier == 2).unsqueeze(1)
    nxt = (y + 1) % C
    t.scatter_(1, nxt, torch.where(tie, (a + 30.0).unsqueeze(1), t.gather(1, nxt)))
    return t.contiguous()
