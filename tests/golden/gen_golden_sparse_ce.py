"""Generate the golden vectors of the label-map cross-entropy from the reference's lovasz.xloss.

RUNS ONLY WHERE THE REFERENCE IS MOUNTED (same convention as gen_golden_lovasz.py: /root/reference on sys.path).  It
calls the reference's `lovasz.xloss` (F.cross_entropy(logits, labels, ignore_index=255), lovasz.py:223-227) in fp32 on
the CPU and writes tests/golden/sparse_ce_<name>.npz: the logits, the label map, the loss, and d (loss * w) / d logits
under a fixed upstream weight w.  The fixtures are data; nothing from the reference travels with them.

  s1        3x3x23x29 (odd HW, no multiple of a wave), about a tenth of the pixels void (255)
  c19       2x19x16x16 (many classes), void pixels, the second image entirely void
  novoid    2x5x8x8, every pixel labelled
  allvoid   1x4x6x6, every pixel void: the loss is NaN, the gradient zero

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_sparse_ce.py
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

torch.set_num_threads(8)
W = 0.7312


def emit(name, x, y):
    x = x.clone().requires_grad_(True)
    loss = lovasz.xloss(x, y)
    (loss * W).backward()
    path = os.path.join(OUT, f'sparse_ce_{name}.npz')
    np.savez_compressed(path, x=x.detach().numpy(), y=y.numpy().astype(np.uint8), w=np.float32(W),
                        loss=loss.detach().numpy(), grad=x.grad.numpy(), torch_version=np.asarray(torch.__version__))
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print(f'{name}: loss {float(loss)!r}  {os.path.getsize(path) / 1024:.1f} KiB')


def case(shape, void, seed):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W_ = shape
    x = 3 * torch.randn(shape, generator=g)
    y = torch.randint(0, C, (B, H, W_), generator=g)
    y[torch.rand(B, H, W_, generator=g) < void] = 255
    return x, y


if __name__ == '__main__':
    emit('s1', *case((3, 3, 23, 29), 0.1, 1))
    x, y = case((2, 19, 16, 16), 0.2, 2)
    y[1] = 255
    emit('c19', x, y)
    emit('novoid', *case((2, 5, 8, 8), 0.0, 3))
    emit('allvoid', *case((1, 4, 6, 6), 1.1, 4))
