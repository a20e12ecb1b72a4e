"""Generate the golden vectors of the losses beyond BCE / Lovász / RMI from the reference's losses.py.

RUNS ONLY WHERE THE REFERENCE IS MOUNTED (same convention as gen_golden.py: /root/reference on sys.path, an empty
`kornia` stub).  It calls the reference's `losses` module in fp32 on the CPU and writes
tests/golden/losses_ext_<name>.npz: the inputs, the loss, and d (loss * w).sum() / d input under a fixed non-trivial
upstream weight w.  The fixtures are data; nothing from the reference travels with them.

Shapes: S1 = 3x3x23x29 (odd HW, no multiple of a wave or a block, C != 2), S2 = 2x21x16x16 (many classes),
S3 = 4x2x64x64 (more than one reduction partial).  OHEM runs at 2x3x24x24 (n = 1152) in three regimes.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_losses.py
"""
import os
import sys
import types

import numpy as np

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.modules.setdefault('kornia', types.ModuleType('kornia'))

import torch  # noqa: E402

import losses  # noqa: E402  (reference)

torch.set_num_threads(8)
S1, S2, S3 = (3, 3, 23, 29), (2, 21, 16, 16), (4, 2, 64, 64)
SHAPES = {'s1': S1, 's2': S2, 's3': S3}


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    out['torch_version'] = np.asarray(torch.__version__)
    path = os.path.join(OUT, f'losses_ext_{name}.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print(f'{name}: {os.path.getsize(path) / 1024:.0f} KiB')


def logits(shape, scale=2.0):
    return torch.randn(shape) * scale


def onehot(shape):
    B, C, H, W = shape
    lab = torch.randint(0, C, (B, H, W))
    return torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).contiguous().float()


def run(fn, x, *rest):
    """loss, the upstream weight w, and d (loss * w).sum() / d x"""
    x = x.clone().requires_grad_(True)
    loss = fn(x, *rest)
    w = torch.tensor(0.7312) if loss.dim() == 0 else torch.randn(loss.shape) * 0.5 + 1.0
    (loss * w).sum().backward()
    return loss.detach(), w, x.grad.detach()


def gen_ce():
    for key, shape in SHAPES.items():
        x, t = logits(shape), onehot(shape)
        loss, w, g = run(losses.DenseCrossEntropyLossWithLogits('mean'), x, t)
        save(f'ce_mean_{key}', x=x, t=t, w=w, loss=loss, grad=g)
    x, t = logits(S1), losses.smooth_labels(onehot(S1), 0.1)
    loss, w, g = run(losses.DenseCrossEntropyLossWithLogits('mean'), x, t)
    save('ce_mean_soft', x=x, t=t, w=w, loss=loss, grad=g)
    x, t = logits(S1), onehot(S1)
    loss, w, g = run(losses.DenseCrossEntropyLossWithLogits('none'), x, t)
    save('ce_none_s1', x=x, t=t, w=w, loss=loss, grad=g)


def gen_focal():
    for key, shape in SHAPES.items():
        x, t = logits(shape), onehot(shape)
        loss, w, g = run(losses.FocalLoss(), x, t)
        save(f'focal_{key}', x=x, t=t, w=w, loss=loss, grad=g, alpha=0.25, gamma=2.0)
    x, t = logits(S1), losses.smooth_labels(onehot(S1), 0.1)
    loss, w, g = run(losses.FocalLoss(0.5, 2), x, t)
    save('focal_soft', x=x, t=t, w=w, loss=loss, grad=g, alpha=0.5, gamma=2.0)
    x, t = logits(S1), onehot(S1)
    loss, w, g = run(losses.FocalLoss(0.25, 1.5), x, t)
    save('focal_g15', x=x, t=t, w=w, loss=loss, grad=g, alpha=0.25, gamma=1.5)
    # saturated logits, gamma = 2: the gradient there is 0 (right side) or alpha_t (wrong side), never NaN
    x, t = logits(S1), onehot(S1)
    x.view(-1)[::7] = 100.0
    x.view(-1)[3::11] = -100.0
    loss, w, g = run(losses.FocalLoss(), x, t)
    assert torch.isfinite(g).all()
    save('focal_sat', x=x, t=t, w=w, loss=loss, grad=g, alpha=0.25, gamma=2.0)


def gen_ohem():
    shape, thres = (2, 3, 24, 24), 0.7
    torch.manual_seed(0)
    x, t = logits(shape), onehot(shape)
    n = shape[0] * shape[2] * shape[3]
    for min_kept, want in ((100, 928), (1000, 1000), (5000, 1151)):
        loss, w, g = run(losses.OhemCrossEntropy(thres, min_kept), x, t)
        kept = None
        for dt in (torch.float32, torch.float64):
            pred = torch.softmax(x.to(dt), 1).gather(1, t.argmax(1, keepdim=True)).view(-1).sort()[0]
            k = min(min_kept, n - 1)
            thr = max(float(pred[k]), thres)
            near = int(((pred - thr).abs() < 1e-5).sum())
            # nobody but the order-statistic pixel itself sits within 1e-5 of the threshold
            assert near == (1 if float(pred[k]) >= thres else 0), (min_kept, dt, near)
            cnt = int((pred < thr).sum())
            assert kept in (None, cnt)
            kept = cnt
        assert kept == want, (min_kept, kept, want)
        save(f'ohem_k{min_kept}', x=x, t=t, w=w, loss=loss, grad=g, thres=thres, min_kept=min_kept, kept=kept,
             threshold=np.float32(max(float(torch.softmax(x, 1).gather(1, t.argmax(1, keepdim=True)).view(-1)
                                            .sort()[0][min(min_kept, n - 1)]), thres)))


def gen_dice():
    for key, shape in SHAPES.items():
        x, t = logits(shape), onehot(shape)
        loss, w, g = run(losses.DiceWithLogitsLoss(), x, t)
        assert torch.isfinite(loss)
        save(f'dice_{key}', x=x, t=t, w=w, loss=loss, grad=g)
    # sample 0 without class 2 (mask 0 for that class)
    x, t = logits(S1), onehot(S1)
    t[0, 0] += t[0, 2]
    t[0, 2] = 0
    loss, w, g = run(losses.DiceWithLogitsLoss(), x, t)
    assert torch.isfinite(loss)
    save('dice_absent', x=x, t=t, w=w, loss=loss, grad=g)
    # sample 1 empty: no class present, the masked mean is 0/0
    x, t = logits(S1), onehot(S1)
    t[1] = 0
    loss, w, g = run(losses.DiceWithLogitsLoss(), x, t)
    assert torch.isnan(loss)
    save('dice_nan', x=x, t=t, w=w, loss=loss, grad=g)


def nfl_labels(shape, strip_samples):
    lab = (torch.rand(shape) > 0.6).float()
    for b in strip_samples:
        lab[b, :, 2:5, :] = -1.0
    return lab


def gen_nfl():
    cases = {
        'nfl_default': (S1, dict(), (1,)),
        'nfl_s2': (S2, dict(alpha=0.5, gamma=2, scale=2.0, weight=0.5), (0,)),
        'nfl_logits': (S3, dict(from_logits=True, size_average=False, gamma=1.5, eps=1e-6), (0, 1, 2, 3)),
        'nfl_sum': (S1, dict(size_average=False), ()),
    }
    for name, (shape, kw, strips) in cases.items():
        m = losses.NormalizedFocalLossSigmoid(**kw)
        xs, ls, ks = [], [], []
        for call in range(2):
            x = torch.rand(shape) * 0.98 + 0.01 if kw.get('from_logits') else logits(shape)
            lab = nfl_labels(shape, strips)
            if call == 0:
                loss, w, g = run(m, x, lab)
            else:
                loss2 = m(x, lab).detach()
            xs.append(x)
            ls.append(lab)
            ks.append(float(m._k_sum))
        if len(strips) == shape[0]:
            assert ks == [0.0, 0.0]      # every sample has a -1 label: the update is skipped
        full = dict(axis=-1, alpha=0.25, gamma=2, from_logits=False, weight=1.0, size_average=True, eps=1e-12,
                    scale=1.0, ignore_label=-1)
        full.update(kw)
        save(name, x=xs[0], t=ls[0], w=w, loss=loss, grad=g, x2=xs[1], t2=ls[1], loss2=loss2, k_sum=np.asarray(ks),
             **{'p_' + k: v for k, v in full.items()})


def gen_dice_prob():
    x, t = torch.sigmoid(logits(S1)), onehot(S1)
    loss, w, g = run(losses.dice_loss, x, t)
    save('dicep_s1', x=x, t=t, w=w, loss=loss, grad=g)
    loss, w, g = run(losses.log_dice_loss, x, t)
    save('logdicep_s1', x=x, t=t, w=w, loss=loss, grad=g, gamma=1.0)
    x, t = torch.sigmoid(logits(S3)), onehot(S3)
    loss, w, g = run(lambda a, b: losses.log_dice_loss(a, b, gamma=2.0), x, t)
    save('logdicep_g2', x=x, t=t, w=w, loss=loss, grad=g, gamma=2.0)


def gen_entropy():
    x = logits(S1).clamp(-10, 10)
    loss, w, g = run(losses.binary_entropy_loss, x)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    save('bent_in', x=x, w=w, loss=loss, grad=g)
    x = logits(S1).clamp(-10, 10)
    x[1, 2, 5, 7] = 30.0
    loss, w, g = run(losses.binary_entropy_loss, x)
    assert torch.isnan(loss)
    save('bent_nan', x=x, w=w, loss=loss, grad=g)
    for key, shape in SHAPES.items():
        x = logits(shape)
        loss, w, g = run(losses.entropy_loss, x)
        save(f'ent_{key}', x=x, w=w, loss=loss, grad=g)


def gen_bce():
    for red in ('none', 'sum'):
        x, t = logits(S1), onehot(S1)
        loss, w, g = run(losses.DenseBinaryCrossEntropyLossWithLogits(red), x, t)
        save(f'bce_{red}_s1', x=x, t=t, w=w, loss=loss, grad=g)


def gen_smooth():
    t = onehot(S2)
    save('smooth_s2', t=t, out=losses.smooth_labels(t, 0.1), alpha=0.1)
    assert losses.get_dims_with_exclusion(4, 0) == [1, 2, 3]


if __name__ == '__main__':
    for i, gen in enumerate((gen_ohem, gen_ce, gen_focal, gen_dice, gen_nfl, gen_dice_prob, gen_entropy, gen_bce,
                             gen_smooth)):
        torch.manual_seed(100 + i)
        gen()
