"""Losses — drop-in for the reference's losses.py, on the MI355X kernels.

  CalculateLoss                           losses.py:8-22   (bilinear resize of each prediction + weighted sum)
  DenseCrossEntropyLossWithLogits         losses.py:25-39  (reduction 'mean' / 'none', soft targets)
  DenseBinaryCrossEntropyLossWithLogits   losses.py:41-48  (reduction 'mean' / 'sum' / 'none')
  OhemCrossEntropy                        losses.py:51-69  (order statistic by a device radix select, no host sync;
                                          a [B, H, W] target is a label map with a void label)
  CrossEntropyLossWithLogits              lovasz.py:227    (F.cross_entropy on a [B, H, W] label map: void label, class
                                          weights, label smoothing; lovasz.xloss itself keeps raising)
  FocalLoss                               losses.py:72-90
  NormalizedFocalLossSigmoid              losses.py:93-151 (detach_delimeter=True, scalar weight; _k_sum on the device)
  DiceWithLogitsLoss                      losses.py:157-167
  get_dims_with_exclusion                 losses.py:213-218
  dice_loss, log_dice_loss                losses.py:221-236
  binary_lovasz_loss_with_logits          losses.py:239-250
  LovaszSoftmaxLossWithLogits             lovasz.py:155-201 on logits, softmax fused (any C <= 64, classes, ignore)
  LovaszHingeLossWithLogits               lovasz.py:79-112 on one-channel logits
  binary_entropy_loss, entropy_loss       losses.py:253-264
  smooth_labels                           losses.py:267-268
  RMILoss                                 losses.py:271-592 (the default-config loss, configs/default_config.py:147;
                                          sigmoid form, rmi_pool 'avg' / 'none', rmi_radius 1-3)
Every loss runs in csrc/eltwise.hip, lovasz.hip, rmi.hip or seglosses.hip; there is no framework fallback.
"""
import torch
import torch.nn as nn

from ssseg import native as N
from ssseg import ops


class CalculateLoss:
    def __init__(self, losses):
        # losses: list of {'loss_fn': callable(prediction, target), 'weight': [w per prediction]}
        self.losses = losses

    def __call__(self, predictions_list, target):
        total = None
        size = tuple(target.shape[-2:])   # [B, C, H, W] targets and [B, H, W] label maps alike
        for idx, prediction in enumerate(predictions_list):
            prediction = ops.interpolate_bilinear(prediction, size, align_corners=False)
            for spec in self.losses:
                term, w = spec['loss_fn'](prediction, target), float(spec['weight'][idx])
                # total + term * w on the device (ssseg_axpby): same fp32 arithmetic as the reference's
                total = ops.scale(term, w) if total is None else ops.add_scaled(total, term, w)
        return total if total is not None else 0


class DenseCrossEntropyLossWithLogits(nn.Module):
    def __init__(self, reduction='mean'):
        super().__init__()
        self.reduction = reduction

    def forward(self, input, target):
        if self.reduction not in ('mean', 'none'):
            raise ValueError(f'incorrect value of reduction param: `{self.reduction}`')
        return ops.dense_cross_entropy(input, target, self.reduction)


class DenseBinaryCrossEntropyLossWithLogits(nn.Module):
    def __init__(self, reduction='mean'):
        super().__init__()
        self.reduction = reduction

    def forward(self, input, target):
        if self.reduction == 'mean':
            return ops.bce_with_logits_mean(input, target)
        if self.reduction not in ('sum', 'none'):
            raise ValueError(f'{self.reduction} is not a valid value for reduction')
        return ops.bce_with_logits(input, target, self.reduction)


class CrossEntropyLossWithLogits(nn.Module):
    """nn.CrossEntropyLoss on a label map: logits [B, C, H, W] (2 <= C <= 64) against labels [B, H, W] (uint8 or
    int64, read in place) with a void label, optional class weights and label smoothing: the F.cross_entropy call of
    the reference's lovasz.xloss (lovasz.py:227), which lovasz.xloss itself still refuses here.  A label outside
    [0, C) that is not ignore_index counts as void too (torch raises on it; the kernels cannot without a host sync).
    empty: what 'mean' gives when every pixel is void, 'nan' like torch or 'zero'."""

    def __init__(self, weight=None, ignore_index=255, reduction='mean', label_smoothing=0.0, empty='nan'):
        super().__init__()
        self.register_buffer('weight', None if weight is None else torch.as_tensor(weight, dtype=torch.float32))
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        self.empty = empty

    def forward(self, input, target):
        weight = self.weight
        if weight is not None and weight.device != input.device:
            weight = self.weight = weight.to(input.device)
        return ops.cross_entropy_labels(input, target, weight, self.ignore_index, self.reduction,
                                        self.label_smoothing, self.empty)


class OhemCrossEntropy(nn.Module):
    """losses.py:51-69.  A target [B, H, W] is a label map (uint8 / int64) whose ignore_label pixels are void, as in
    the HRNet original the reference's class was taken from; a [B, C, H, W] target takes the dense path."""

    def __init__(self, thres=0.7, min_kept=100000, ignore_label=255):
        super().__init__()
        self.thresh = thres
        self.min_kept = max(1, min_kept)
        self.ignore_label = ignore_label
        self.criterion = DenseCrossEntropyLossWithLogits(reduction='none')

    def forward(self, logits, target):
        if target.dim() == logits.dim() - 1:
            return ops.ohem_cross_entropy_labels(logits, target, self.thresh, self.min_kept, self.ignore_label)
        return ops.ohem_cross_entropy(logits, target, self.thresh, self.min_kept)


class FocalLoss(nn.Module):
    def __init__(self, alpha=0.25, gamma=2.0):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma

    def forward(self, inputs, targets):
        return ops.focal_loss(inputs, targets, self.alpha, self.gamma)


class NormalizedFocalLossSigmoid(nn.Module):
    """losses.py:93-151.  The reference keeps `_k_sum` as a host float and reads two tensors back per call; here it is
    a device scalar that the final kernel of the forward updates under the same rule (`float(loss._k_sum)` works), so
    the forward never synchronises.  detach_delimeter=False (on which the reference itself raises, losses.py:136) and
    a tensor `weight` are refused at construction."""

    def __init__(self, axis=-1, alpha=0.25, gamma=2, from_logits=False, batch_axis=0, weight=None, size_average=True,
                 detach_delimeter=True, eps=1e-12, scale=1.0, ignore_label=-1):
        super().__init__()
        if not detach_delimeter:
            raise NotImplementedError('NormalizedFocalLossSigmoid: detach_delimeter=False (the reference raises on it)')
        if isinstance(weight, torch.Tensor):
            raise NotImplementedError('NormalizedFocalLossSigmoid: a tensor `weight` (the kernel takes a scalar)')
        self._axis = axis
        self._alpha = alpha
        self._gamma = gamma
        self._ignore_label = ignore_label
        self._weight = weight if weight is not None else 1.0
        self._batch_axis = batch_axis
        self._scale = scale
        self._from_logits = from_logits
        self._eps = eps
        self._size_average = size_average
        self._detach_delimeter = detach_delimeter
        self._k_sum = 0

    def forward(self, pred, label, sample_weight=None):
        if not isinstance(self._k_sum, torch.Tensor):
            self._k_sum = torch.full((), float(self._k_sum), device=pred.device, dtype=torch.float32)
        params = N.NflParams(self._alpha, self._gamma, self._eps, self._scale, self._weight, self._ignore_label,
                             int(bool(self._from_logits)), int(bool(self._size_average)))
        return ops.normalized_focal_loss(pred, label, params, self._k_sum)

    def log_states(self, sw, name, global_step):
        sw.add_scalar(tag=name + '_k', value=float(self._k_sum), global_step=global_step)


class DiceWithLogitsLoss(nn.Module):
    def forward(self, input, target):
        return ops.dice_with_logits(input, target)


def get_dims_with_exclusion(dim, exclude=None):
    dims = list(range(dim))
    if exclude is not None:
        dims.remove(exclude)
    return dims


def dice_loss(input, target):
    """losses.py:221-227 on probabilities: per-sample 1 - (2 I + 1) / (K + 1)."""
    return ops.dice_prob(input, target, log_mode=False)


def log_dice_loss(input, target, gamma=1.0):
    """losses.py:230-236: per-sample (-log((2 I + 1) / (K + 1))) ** gamma."""
    return ops.dice_prob(input, target, log_mode=True, gamma=gamma)


def binary_entropy_loss(input):
    """losses.py:253-257, literally: sigmoid, then log (NaN where the fp32 sigmoid saturates, as in the reference)."""
    return ops.binary_entropy(input)


def entropy_loss(input):
    """losses.py:260-264."""
    return ops.entropy(input)


def smooth_labels(target, alpha=0.1):
    """losses.py:267-268: target * (1 - alpha) + alpha / C."""
    return ops.smooth_labels(target, alpha)


def binary_lovasz_loss_with_logits(input, target):
    """losses.py:239-250: per-image binary Lovász-softmax on raw logits (class 1), sum(loss*valid)/(sum valid + 0.001)."""
    return ops.lovasz_binary(input, target)


class LovaszSoftmaxLossWithLogits(nn.Module):
    """Multi-class Lovász-softmax (lovasz.lovasz_softmax) on raw logits [B, C, H, W] against a one-hot or soft target
    of the same shape: the label of a pixel is the argmax of its target (as in binary_lovasz_loss_with_logits), read
    inside the kernels; the softmax over C is fused into them.  A target [B, H, W] is taken as the label map itself
    (int64 or uint8, read in place).  classes: 'present', 'all' or a list of class ids; ignore: the label value of void
    pixels (only a label map can hold the default 255: an argmax over C <= 64 channels never reaches it)."""

    def __init__(self, classes='present', per_image=False, ignore=255):
        super().__init__()
        if isinstance(classes, str) and classes not in ('all', 'present'):
            raise ValueError(f"classes must be 'all', 'present' or a list of class ids, got {classes!r}")
        self.classes = classes
        self.per_image = per_image
        self.ignore = ignore

    def forward(self, input, target):
        if input.dim() != 4 or input.shape[1] < 2:
            raise ValueError(f'LovaszSoftmaxLossWithLogits: expected logits [B, C >= 2, H, W], got {tuple(input.shape)}')
        if isinstance(self.classes, str):
            ids, present = list(range(input.shape[1])), self.classes == 'present'
        else:
            ids, present = list(self.classes), False
        return ops.lovasz_general(input, target, N.LOVASZ_SOFTMAX, ids, self.per_image, self.ignore, present,
                                  dense_target=target.dim() == input.dim())


class LovaszHingeLossWithLogits(nn.Module):
    """Binary Lovász hinge (lovasz.lovasz_hinge) on one-channel logits [B, 1, H, W] against a 0 / 1 mask of the same
    number of pixels ([B, 1, H, W] or [B, H, W]; float masks are read in place); ignore: the mask value of void
    pixels, None for no void."""

    def __init__(self, per_image=True, ignore=None):
        super().__init__()
        self.per_image = per_image
        self.ignore = ignore

    def forward(self, input, target):
        if input.dim() != 4 or input.shape[1] != 1:
            raise ValueError(f'LovaszHingeLossWithLogits: expected logits [B, 1, H, W], got {tuple(input.shape)}')
        return ops.lovasz_general(input, target, N.LOVASZ_HINGE, [1], self.per_image, self.ignore)


class RMILoss(nn.Module):
    """Region mutual information loss (losses.py:271-592), forward = forward_sigmoid (losses.py:480-518).

    Same constructor and checks as the reference (:286-311).  The device kernels (csrc/rmi.hip) cover the pools the
    reference's configs use ('avg', and 'none') and rmi_radius 1-3 (D = radius^2 <= 9; the default config uses 3);
    'max' / 'interpolation' pooling and larger radii raise NotImplementedError here rather than run elsewhere."""

    _CLIP_MIN = 1e-6    # losses.py:281-283
    _CLIP_MAX = 1.0
    _POS_ALPHA = 5e-4
    _IS_SUM = 1

    def __init__(self, num_classes=21, rmi_radius=3, rmi_pool='avg', rmi_pool_size=3, rmi_pool_stride=3):
        super().__init__()
        self.num_classes = num_classes
        assert rmi_radius in [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
        self.rmi_radius = rmi_radius
        assert rmi_pool in ['max', 'avg', 'interpolation', 'none']
        self.rmi_pool = rmi_pool
        assert rmi_pool_size == rmi_pool_stride
        self.rmi_pool_size = rmi_pool_size
        self.rmi_pool_stride = rmi_pool_stride
        self.half_d = rmi_radius * rmi_radius
        self.d = 2 * self.half_d
        self.kernel_padding = rmi_pool_size // 2
        self.ignore_index = 255
        if rmi_radius > 3:
            raise NotImplementedError(f'RMILoss: rmi_radius={rmi_radius} (kernels cover 1-3, D <= 9)')
        if rmi_pool_stride > 1 and rmi_pool in ('max', 'interpolation'):
            raise NotImplementedError(f'RMILoss: rmi_pool={rmi_pool!r} (kernels cover avg and none)')

    def pool_params(self):
        """(k, s, pad) of losses.py:529-538; (1, 1, 0) when the reference skips the pooling."""
        if self.rmi_pool_stride <= 1 or self.rmi_pool == 'none':
            return 1, 1, 0
        return self.rmi_pool_size, self.rmi_pool_stride, self.kernel_padding

    def forward(self, logits_4D, labels_4D):
        return ops.rmi_loss(logits_4D, labels_4D, self.num_classes, self.rmi_radius, *self.pool_params())
