"""Synthetic labeled / unlabeled segmentation datasets for the BASELINE configs: images
U[0,1) and 2-channel one-hot masks of smoothed-noise blobs.  The reference's SkinSegDataset needs
cv2 + albumentations (absent here).  num_classes > 2 gives C-channel one-hot masks: the same
smoothed field cut at C - 1 quantiles into nested level sets (background fg_fraction-complement, the rest shared
equally by classes 1 .. C-1).  label_map=True gives the [H, W] label map itself (uint8 by default) instead of the
one-hot, with a share void_fraction of the pixels set to ignore_label: the void pixels come from a generator of their
own, so images and class labels are those of the one-hot dataset of the same seed."""
import math

import torch
import torch.nn.functional as F


class SyntheticSegDataset(torch.utils.data.Dataset):
    def __init__(self, length=64, size=512, seed=0, with_masks=True, blob_sigma=16.0, fg_fraction=0.4, uint8=False,
                 num_classes=2, label_map=False, void_fraction=0.0, ignore_label=255, label_dtype=torch.uint8):
        self.length, self.size, self.seed = length, size, seed
        self.with_masks, self.sigma, self.fg = with_masks, blob_sigma, fg_fraction
        # uint8: the image as the reference's host loader leaves it before ToFloat (LongestMaxSize + PadIfNeeded
        # output, data/dataset.py:70-72), for the device augmentation pipeline (data.device_augment)
        self.uint8 = uint8
        if int(num_classes) < 2:
            raise ValueError(f'SyntheticSegDataset: num_classes must be at least 2, got {num_classes}')
        self.num_classes = int(num_classes)
        if not 0.0 <= float(void_fraction) <= 1.0:
            raise ValueError(f'SyntheticSegDataset: void_fraction must lie in [0, 1], got {void_fraction}')
        if void_fraction and not label_map:
            raise ValueError('SyntheticSegDataset: void pixels need label_map=True (a one-hot mask cannot hold them)')
        self.label_map, self.void_fraction = bool(label_map), float(void_fraction)
        self.ignore_label, self.label_dtype = int(ignore_label), label_dtype

    def __len__(self):
        return self.length

    def _blobs(self, g, labels=False):
        k = int(2 * round(3 * self.sigma) + 1)
        x = torch.arange(k, dtype=torch.float32) - k // 2
        w = torch.exp(-x * x / (2 * self.sigma ** 2))
        w = (w / w.sum()).view(1, 1, k, 1)
        n = torch.randn(1, 1, self.size, self.size, generator=g)
        f = F.conv2d(F.conv2d(n, w, padding=(k // 2, 0)), w.transpose(2, 3), padding=(0, k // 2))
        if self.num_classes == 2:
            thr = torch.quantile(f.flatten(), 1 - self.fg)
            return (f > thr)[0, 0].long() if labels else (f > thr).float()[0]
        # C classes: level k (1 <= k < C) starts at the quantile 1 - fg * (C - k) / (C - 1) of the field
        C = self.num_classes
        q = torch.tensor([1 - self.fg * (C - k) / (C - 1) for k in range(1, C)], dtype=torch.float32)
        thr = torch.quantile(f.flatten(), q)
        label = (f[0] > thr.view(-1, 1, 1)).sum(0)                       # [size, size] in [0, C)
        return label if labels else F.one_hot(label, C).permute(2, 0, 1).float()

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + i)
        out = {'image': torch.rand(3, self.size, self.size, generator=g)}
        if self.uint8:
            out['image'] = (out['image'] * 255).round().to(torch.uint8)
        if self.with_masks and self.label_map:
            label = self._blobs(g, labels=True)
            if self.void_fraction > 0:
                gv = torch.Generator().manual_seed((1 << 40) + self.seed * 1_000_003 + i)
                label[torch.rand(self.size, self.size, generator=gv) < self.void_fraction] = self.ignore_label
            out['semantic_mask'] = label.to(self.label_dtype)
        elif self.with_masks:
            fg = self._blobs(g)
            out['semantic_mask'] = torch.cat([1 - fg, fg], 0) if self.num_classes == 2 else fg
        return out
