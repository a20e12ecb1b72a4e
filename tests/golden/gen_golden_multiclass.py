"""Generate tests/golden/multiclass_iou.npz from the reference's lovasz.iou.

RUNS ONLY WHERE THE REFERENCE IS MOUNTED (same convention as gen_golden_lovasz.py: /root/reference on sys.path).  It
calls the reference's `lovasz.iou` (lovasz.py:54-73, per_image=False) on small random prediction / label maps and
records the inputs and the returned 100 * IoU arrays.  The fixture is data; nothing from the reference travels with it.

  c2, c3, c19        random predictions against random labels
  c5_absent          class 3 in neither the labels nor the predictions (EMPTY = 1 -> 100)
  c19_ignore         a fifth of the labels are 255, ignore=255

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_multiclass.py
"""
import os
import sys

import numpy as np

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import torch  # noqa: E402

import lovasz  # noqa: E402  (reference)

NONE = -1   # `ignore` stored as -1 when the call passes None


def main():
    g = torch.Generator().manual_seed(20)
    out = {}
    cases = [('c2', 2, None, None), ('c3', 3, None, None), ('c19', 19, None, None), ('c5_absent', 5, 3, None),
             ('c19_ignore', 19, None, 255)]
    for name, C, absent, ignore in cases:
        pred = torch.randint(0, C, (2, 13, 11), generator=g)
        label = torch.randint(0, C, (2, 13, 11), generator=g)
        if absent is not None:
            pred[pred == absent] = 0
            label[label == absent] = 1
        if ignore is not None:
            label[torch.rand(label.shape, generator=g) < 0.2] = ignore
        ious = lovasz.iou(pred, label, C, EMPTY=1., ignore=ignore, per_image=False)
        out[f'{name}.pred'] = pred.numpy().astype(np.int64)
        out[f'{name}.label'] = label.numpy().astype(np.int64)
        out[f'{name}.C'] = np.asarray(C)
        out[f'{name}.ignore'] = np.asarray(NONE if ignore is None else ignore)
        out[f'{name}.iou100'] = np.asarray(ious, np.float64)
        print(name, np.asarray(ious).round(2))
    out['torch_version'] = np.asarray(torch.__version__)
    path = os.path.join(OUT, 'multiclass_iou.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print(f'{path}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
