"""fp64 restatements of the label-map losses (plain PyTorch, CPU): the yardstick of test_sparse_losses_host.py (which
pins it to F.cross_entropy, to the reference's dense OhemCrossEntropy and to the reference's lovasz.xloss fixtures) and
of the GPU tests in test_sparse_losses.py.

Void pixels: the ignore value, and every label outside [0, C) (torch raises on those; the device kernels cannot
without a host sync and treat them as void, so the yardstick does too)."""
import torch


def _split(x, y, ignore):
    """(valid [B,...] bool, labels with void replaced by 0, log-probabilities)"""
    C = x.shape[1]
    y = y.long()
    valid = (y != ignore) & (y >= 0) & (y < C)
    return valid, torch.where(valid, y, torch.zeros_like(y)), torch.log_softmax(x, 1)


def ce_labels64(x, y, weight=None, ignore_index=255, reduction='mean', label_smoothing=0.0, empty='nan'):
    """F.cross_entropy(x, y, weight, ignore_index=..., reduction=..., label_smoothing=...) written out:
    l = (1 - eps) w_y (-logp_y) + eps / C sum_c w_c (-logp_c) per valid pixel, 0 per void pixel; 'mean' divides by
    the sum of w_y over the valid pixels.  Everything void under 'mean': NaN (empty='nan') or 0 (empty='zero'), with
    a zero gradient either way."""
    C, eps = x.shape[1], float(label_smoothing)
    valid, ys, logp = _split(x, y, ignore_index)
    w = torch.ones(C, dtype=x.dtype) if weight is None else weight.to(x.dtype)
    wy = w[ys]
    nll = -logp.gather(1, ys.unsqueeze(1)).squeeze(1)
    smooth = -(logp * w.view([1, C] + [1] * (x.dim() - 2))).sum(1)
    l = ((1 - eps) * wy * nll + eps / C * smooth) * valid
    if reduction == 'none':
        return l
    if reduction == 'sum':
        return l.sum()
    den = (wy * valid).sum()
    if float(den) == 0.0 and not bool(valid.any()):
        return l.sum() * 0 + (0.0 if empty == 'zero' else float('nan'))
    return l.sum() / den


def ohem_labels_state64(x, y, thres, min_kept, ignore_label=255):
    """(threshold, selection mask [B,...], n_valid): pred = softmax at the label; the order statistic
    k = min(min_kept, n_valid - 1) and the threshold max(sorted(pred)[k], thres) over the valid pixels only; kept =
    valid and pred < threshold.  No valid pixel: threshold +inf, nothing kept."""
    valid, ys, logp = _split(x, y, ignore_label)
    pred = torch.softmax(x, 1).gather(1, ys.unsqueeze(1)).squeeze(1)
    flat = pred[valid].sort()[0]
    n = flat.numel()
    if n == 0:
        return float('inf'), torch.zeros_like(valid), 0
    thr = max(float(flat[min(int(min_kept), n - 1)]), float(thres))
    return thr, valid & (pred < thr), n


def ohem_labels64(x, y, thres, min_kept, ignore_label=255):
    """mean CE over the kept pixels (NaN when none is kept); no gradient through the selection"""
    _, sel, _ = ohem_labels_state64(x.detach(), y, thres, min_kept, ignore_label)
    valid, ys, logp = _split(x, y, ignore_label)
    nll = -logp.gather(1, ys.unsqueeze(1)).squeeze(1)
    if not bool(sel.any()):
        return nll.sum() * 0 + float('nan')   # NaN loss, zero gradient
    return (nll * sel).sum() / sel.sum()


def confusion(pred_labels, y, C, ignore):
    """[C, C] int64 confusion matrix (rows label, columns prediction) over the valid pixels"""
    y = y.long().reshape(-1)
    p = pred_labels.long().reshape(-1)
    valid = (y >= 0) & (y < C) if ignore is None else (y != ignore) & (y >= 0) & (y < C)
    return torch.bincount(y[valid] * C + p[valid], minlength=C * C).reshape(C, C)
