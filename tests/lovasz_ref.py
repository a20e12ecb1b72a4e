"""numpy restatement of the general Lovász losses (reference lovasz.py:79-127, 155-220) and of their gradients, for
tests/test_lovasz_general.py and tests/test_lovasz_general_host.py.  Stable descending argsort over the valid pixels of
each group, the fp32 Jaccard steps of oracle.losses_ref.lovasz_grad, an fp64 dot rounded to fp32, fp32 means in index
order (the reference's mean()).  Two cases on which the reference fails are defined as the kernels define them: a
group without a valid pixel contributes 0 loss and zero gradient and still counts in the mean over groups; a group
with one valid pixel follows the formula."""
import numpy as np

from oracle.losses_ref import lovasz_grad

F32 = np.float32


def softmax(x):
    """softmax over axis 1 of fp32 logits, correctly rounded to fp32: exponentials and their sum in fp64"""
    x = np.asarray(x, F32)
    e = np.exp(x.astype(np.float64) - x.max(1, keepdims=True).astype(np.float64))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def class_ids(classes, C):
    """(class ids, present flag) of the reference's `classes` argument"""
    if isinstance(classes, str):
        assert classes in ('all', 'present')
        if C == 1:
            raise ValueError('Sigmoid output possible only with 1 class')
        return list(range(C)), classes == 'present'
    classes = [int(c) for c in classes]
    if C == 1 and len(classes) != 1:
        raise ValueError('Sigmoid output possible only with 1 class')
    return classes, False


def _errors(mode, xc, fg):
    if mode == 'hinge':
        return (F32(1.0) - xc * (F32(2.0) * fg - F32(1.0))).astype(F32) + F32(0.0)
    return np.abs(fg - xc).astype(F32)


def segments(x, labels, mode, classes, per_image, ignore):
    """yields (group, k, channel, pixel indices of the group's valid pixels, fg, err) with x [B, C, HW] (probabilities
    or hinge logits) and labels [B, HW]; pixel indices are into the flat [B*HW] order"""
    B, C, HW = x.shape
    ids, _ = class_ids(classes, C)
    lab = labels.reshape(-1)
    groups = [np.arange(b * HW, (b + 1) * HW) for b in range(B)] if per_image else [np.arange(B * HW)]
    for g, idx in enumerate(groups):
        idx = idx[lab[idx] != ignore] if ignore is not None else idx
        for k, c in enumerate(ids):
            ch = 0 if C == 1 else c
            fg = (lab[idx] == c).astype(F32)
            xc = x[idx // HW, ch, idx % HW]
            yield g, k, ch, idx, fg, _errors(mode, xc, fg)


def lovasz(x, labels, mode='probas', classes='present', per_image=False, ignore=None):
    """(loss, d loss / d x) as fp32.  x [B, C, ...]: probabilities ('probas'), logits with the softmax over C applied
    here ('softmax') or one-channel logits ('hinge', classes=[1]); labels [B, ...] integers."""
    x = np.asarray(x, F32)
    shape = x.shape
    B, C = shape[:2]
    x = x.reshape(B, C, -1)
    HW = x.shape[2]
    labels = np.asarray(labels).astype(np.int64).reshape(B, HW)
    p = softmax(x) if mode == 'softmax' else x
    ids, present = class_ids(classes, C)
    K, G = len(ids), (B if per_image else 1)
    seg_loss = np.zeros((G, K), F32)
    counted = np.zeros((G, K), bool)
    weights = {}
    for g, k, ch, idx, fg, err in segments(p, labels, mode, classes, per_image, ignore):
        counted[g, k] = not (present and fg.sum() == 0)
        if idx.size == 0:
            continue
        perm = np.argsort(-err, kind='stable')
        jg = lovasz_grad(fg[perm])
        es = np.maximum(err[perm], 0) if mode == 'hinge' else err[perm]
        seg_loss[g, k] = F32(np.dot(es.astype(np.float64), jg.astype(np.float64)))
        w = np.zeros(idx.size, np.float64)
        w[perm] = jg
        if mode == 'hinge':
            de = np.where(err > 0, -(2.0 * fg - 1.0), 0.0)      # relu'(e) * de/dx
        else:
            de = -np.sign(fg.astype(np.float64) - p[idx // HW, ch, idx % HW])
        weights[g, k] = (ch, idx, w * de)
    total = F32(0.0)
    dp = np.zeros((B, C, HW), np.float64)
    for g in range(G):
        acc, n = F32(0.0), 0
        for k in range(K):
            if counted[g, k]:
                acc = F32(acc + seg_loss[g, k])
                n += 1
        total = F32(total + (acc / F32(n) if n > 1 else acc))
        for k in range(K):
            if counted[g, k] and (g, k) in weights:
                ch, idx, w = weights[g, k]
                np.add.at(dp, (idx // HW, ch, idx % HW), w / (n * G))
    loss = F32(total / F32(G)) if G > 1 else total
    if mode == 'softmax':
        p64 = p.astype(np.float64)
        dp = p64 * (dp - (p64 * dp).sum(1, keepdims=True))
    return loss, dp.astype(F32).reshape(shape)


def min_error_gap(x, labels, mode='probas', classes='present', per_image=False, ignore=None):
    """the least difference between two valid errors of one segment (0: a tie), over all segments"""
    x = np.asarray(x, F32)
    B, C = x.shape[:2]
    x = x.reshape(B, C, -1)
    labels = np.asarray(labels).astype(np.int64).reshape(B, -1)
    p = softmax(x) if mode == 'softmax' else x
    gap = np.inf
    for _, _, _, idx, _, err in segments(p, labels, mode, classes, per_image, ignore):
        if idx.size > 1:
            gap = min(gap, float(np.diff(np.sort(err.astype(np.float64))).min()))
    return gap
