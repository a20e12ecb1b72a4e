"""Lovász losses — drop-in for reference lovasz.py (Berman 2018, MIT).

Device work (sort + scan + dot) runs in ssseg_lovasz_* (the binary call of losses.py:249) and ssseg_lovasz_gen_*
(multi-class softmax / sigmoid, hinge, 'present' / 'all' / class lists, per image or batch-wide, ignore label); the
small host helpers keep the reference's semantics: lovasz_grad (lovasz.py:19-31), iou_binary / iou (:34-73, the mIoU
of BASELINE's parity report), mean (:235-253).  binary_xloss / StableBCELoss go to the BCE kernel; what has no kernel
raises NotImplementedError (xloss, binary_xloss with a void label).  Nothing falls back to framework kernels.
"""
from itertools import filterfalse as ifilterfalse

import numpy as np
import torch

from ssseg import native as N
from ssseg import ops


def lovasz_grad(gt_sorted):
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.float().cumsum(0)
    union = gts + (1 - gt_sorted).float().cumsum(0)
    jaccard = 1. - intersection / union
    if len(gt_sorted) > 1:
        jaccard[1:] = jaccard[1:] - jaccard[:-1].clone()
    return jaccard


def iou_binary(preds, labels, EMPTY=1., ignore=None, per_image=True):
    if not per_image:
        preds, labels = (preds,), (labels,)
    ious = []
    for pred, label in zip(preds, labels):
        inter = ((label == 1) & (pred == 1)).sum()
        union = ((label == 1) | ((pred == 1) & (label != ignore))).sum()
        ious.append(EMPTY if not union else float(inter) / float(union))
    return 100 * mean(ious)


def iou(preds, labels, C, EMPTY=1., ignore=None, per_image=False):
    if not per_image:
        preds, labels = (preds,), (labels,)
    per = []
    for pred, label in zip(preds, labels):
        row = []
        for c in range(C):
            if c == ignore:
                continue
            inter = ((label == c) & (pred == c)).sum()
            union = ((label == c) | ((pred == c) & (label != ignore))).sum()
            row.append(EMPTY if not union else float(inter) / float(union))
        per.append(row)
    return 100 * np.array([mean(col) for col in zip(*per)])


def _class_spec(classes, C):
    """(class ids, present flag) of the reference's `classes` argument ('all', 'present' or a list)"""
    if isinstance(classes, str):
        if classes not in ('all', 'present'):
            raise ValueError(f"classes must be 'all', 'present' or a list of class ids, got {classes!r}")
        if C == 1:   # the reference's len(classes) > 1 check fires for the strings too (lovasz.py:190-192)
            raise ValueError('Sigmoid output possible only with 1 class')
        return list(range(C)), classes == 'present'
    classes = [int(c) for c in classes]
    if C == 1 and len(classes) != 1:
        raise ValueError('Sigmoid output possible only with 1 class')
    return classes, False


def _as_bchw(probas, labels, name):
    if probas.dim() == 3:   # the output of a sigmoid layer (lovasz.py:208-211)
        probas = probas.unsqueeze(1)
    if probas.dim() != 4:
        raise ValueError(f'{name}: expected probas [B, C, H, W] or [B, H, W], got {tuple(probas.shape)}')
    if tuple(labels.shape) != (probas.shape[0],) + tuple(probas.shape[2:]):
        raise ValueError(f'{name}: labels {tuple(labels.shape)} do not match probas {tuple(probas.shape)}')
    return probas


def lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=None):
    """Multi-class Lovász-softmax (lovasz.py:155-201) on the device, without a host synchronisation.

    probas [B, C, H, W] class probabilities, or [B, H, W] / one channel for a sigmoid output (then `classes` must be a
    one-element list, else ValueError, as in the reference); labels [B, H, W] int64 or uint8, read in place (other
    integer types are converted); classes 'all', 'present' or a list; per_image; ignore: the void label.

    As in the reference, 'all' and a list count absent classes (their loss is the largest error), and 'present' with
    nothing present gives 0.  Two cases on which the reference fails are defined here: a group (image, or the batch)
    with no valid pixel contributes 0 loss and zero gradient and still counts in the mean over groups, and a group
    with exactly one valid pixel follows the formula.  Errors sort stably (ties keep pixel order); the loss does not
    depend on the order inside a tie.  The binary per-image call of losses.py:249 ([B, 2, H, W], classes=[1], no
    ignore) keeps its own entry, ops.lovasz_binary(valid_weighted=False)."""
    probas = _as_bchw(probas, labels, 'lovasz_softmax')
    C = probas.shape[1]
    if per_image and not isinstance(classes, str) and list(classes) == [1] and C == 2 and ignore is None:
        target = torch.stack([(labels == 0), (labels == 1)], 1).to(probas.dtype)
        return ops.lovasz_binary(probas, target, valid_weighted=False)
    ids, present = _class_spec(classes, C)
    return ops.lovasz_general(probas, labels, N.LOVASZ_PROBAS, ids, per_image, ignore, present)


def lovasz_softmax_flat(probas, labels, classes='present'):
    """lovasz.py:173-201: probas [P, C], labels [P], one group.  The kernels read channel planes, so probas is
    transposed to [1, C, P] first (one copy).  An empty input gives 0 with zero gradient."""
    if probas.dim() != 2 or labels.dim() != 1 or labels.shape[0] != probas.shape[0]:
        raise ValueError(f'lovasz_softmax_flat: expected probas [P, C] and labels [P], got {tuple(probas.shape)} and '
                         f'{tuple(labels.shape)}')
    ids, present = _class_spec(classes, probas.shape[1])
    if probas.shape[0] == 0:
        return ops.scale(probas.sum(), 0.0)
    return ops.lovasz_general(probas.t().unsqueeze(0), labels.unsqueeze(0), N.LOVASZ_PROBAS, ids, False, None, present)


def lovasz_hinge(logits, labels, per_image=True, ignore=None):
    """Binary Lovász hinge (lovasz.py:79-112) on the device: logits [B, H, W], labels [B, H, W] of 0 / 1 (and
    `ignore`).  Errors 1 - logit * (2 * label - 1) sort descending, the Jaccard gradient runs over all valid pixels and
    the dot takes relu(error).  An image (or batch) with only void pixels contributes 0 with zero gradient, as
    lovasz_hinge_flat does, and counts in the mean over images."""
    if logits.dim() == 4 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.dim() != 3 or tuple(labels.shape) != tuple(logits.shape):
        raise ValueError(f'lovasz_hinge: expected logits and labels [B, H, W], got {tuple(logits.shape)} and '
                         f'{tuple(labels.shape)}')
    return ops.lovasz_general(logits.unsqueeze(1), labels, N.LOVASZ_HINGE, [1], per_image, ignore)


def lovasz_hinge_flat(logits, labels):
    """lovasz.py:95-112: logits [P], labels [P] of 0 / 1, one group; an empty input gives 0 with zero gradient."""
    if logits.dim() != 1 or tuple(labels.shape) != tuple(logits.shape):
        raise ValueError(f'lovasz_hinge_flat: expected logits [P] and labels [P], got {tuple(logits.shape)} and '
                         f'{tuple(labels.shape)}')
    if logits.shape[0] == 0:
        return ops.scale(logits.sum(), 0.0)
    return ops.lovasz_general(logits.view(1, 1, -1), labels.view(1, -1), N.LOVASZ_HINGE, [1], False, None)


def flatten_probas(probas, labels, ignore=None):
    """lovasz.py:204-220: [B, C, H, W] -> ([P, C], [P]) with the void pixels removed.  The output's size depends on
    the labels, so with `ignore` this helper synchronises with the host (boolean indexing); the losses above do not
    use it, they take `ignore` themselves."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)
    C = probas.shape[1]
    probas = probas.permute(0, 2, 3, 1).reshape(-1, C)
    labels = labels.reshape(-1)
    if ignore is None:
        return probas, labels
    valid = labels != ignore
    return probas[valid], labels[valid]


def flatten_binary_scores(scores, labels, ignore=None):
    """lovasz.py:115-127: flat scores and labels with the void pixels removed (synchronises when `ignore` is set, like
    flatten_probas)."""
    scores = scores.reshape(-1)
    labels = labels.reshape(-1)
    if ignore is None:
        return scores, labels
    valid = labels != ignore
    return scores[valid], labels[valid]


class StableBCELoss(torch.nn.Module):
    """lovasz.py:130-137: mean(max(x, 0) - x * t + log(1 + exp(-|x|))), the arithmetic of ssseg_bce_logits_fwd."""

    def forward(self, input, target):
        return ops.bce_with_logits_mean(input, target)


def binary_xloss(logits, labels, ignore=None):
    """lovasz.py:140-149 through the BCE kernel.  The kernel averages over every pixel, so a void label is refused."""
    if ignore is not None:
        raise NotImplementedError('binary_xloss: `ignore` (the BCE kernel takes the mean over all pixels; drop the '
                                  'void pixels with flatten_binary_scores first)')
    return ops.bce_with_logits_mean(logits, labels.float())


def xloss(logits, labels, ignore=None):
    """lovasz.py:223-227 is F.cross_entropy(logits, labels, ignore_index=255) on integer labels.  The CE kernel
    (DenseCrossEntropyLossWithLogits) takes a dense target and the mean over all pixels, so integer `labels` with a
    void index have no kernel here."""
    raise NotImplementedError('xloss: integer `labels` with ignore_index=255 (the CE kernel takes a dense [B, C, H, W] '
                              'target: use losses.DenseCrossEntropyLossWithLogits)')


def isnan(x):
    return x != x


def mean(values, ignore_nan=False, empty=0):
    it = iter(values)
    if ignore_nan:
        it = ifilterfalse(isnan, it)
    try:
        n = 1
        acc = next(it)
    except StopIteration:
        if empty == 'raise':
            raise ValueError('Empty mean')
        return empty
    for n, v in enumerate(it, 2):
        acc += v
    return acc if n == 1 else acc / n
