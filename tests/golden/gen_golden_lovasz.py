"""Generate the golden vectors of the general Lovász losses from the reference's lovasz.py.

RUNS ONLY WHERE THE REFERENCE IS MOUNTED (same convention as gen_golden_losses.py: /root/reference on sys.path).  It
calls the reference's `lovasz` module in fp32 on the CPU (its torch.dot refuses fp64 against the .float() gradient)
and writes tests/golden/lovasz_gen_<name>.npz: the inputs, the configuration, the loss, and d (loss * w) / d input
under a fixed upstream weight w.  The fixtures are data; nothing from the reference travels with them.

  sm_present_batch  softmax probabilities 2x3x5x7, three void pixels (255), classes='present', batch-wide
  sm_all_image      the same inputs, classes='all', per image
  sm_list_image     classes=[1, 2], per image, no void pixels, ignore=None
  absent_present    class 2 absent from the label map, 'present', batch-wide
  absent_all        the same inputs, 'all' (the absent class counts: its loss is the largest error)
  hinge_image       lovasz_hinge 2x5x7 with void pixels, per image
  hinge_batch       the same inputs, batch-wide
  hinge_allvoid     lovasz_hinge 3x5x7 per image, the second image all void
  sigmoid           3-D probabilities 2x5x7 (a sigmoid output), classes=[1], batch-wide, void pixels

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lovasz.py
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
NONE = -1   # `ignore` stored as -1 when the call passes None


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    out['torch_version'] = np.asarray(torch.__version__)
    path = os.path.join(OUT, f'lovasz_gen_{name}.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')


def run(fn, x, labels, **kw):
    x = x.clone().requires_grad_(True)
    loss = fn(x, labels, **kw)
    (loss * W).backward()
    return loss.detach(), x.grad.detach()


def emit(name, mode, x, labels, classes, per_image, ignore):
    kw = dict(per_image=per_image, ignore=ignore)
    if mode == 'hinge':
        loss, grad = run(lovasz.lovasz_hinge, x, labels, **kw)
    else:
        loss, grad = run(lovasz.lovasz_softmax, x, labels, classes=classes, **kw)
    save(name, x=x, labels=labels, mode=mode, classes=np.asarray(classes), per_image=per_image,
         ignore=NONE if ignore is None else ignore, w=W, loss=loss, grad=grad)


def main():
    torch.manual_seed(20)
    B, C, H, Wd = 2, 3, 5, 7
    probas = torch.softmax(torch.randn(B, C, H, Wd) * 2, 1)
    labels = torch.randint(0, C, (B, H, Wd))
    void = labels.clone()
    void[0, 1, 2] = void[0, 4, 6] = void[1, 0, 0] = 255
    emit('sm_present_batch', 'probas', probas, void, 'present', False, 255)
    emit('sm_all_image', 'probas', probas, void, 'all', True, 255)
    emit('sm_list_image', 'probas', probas, labels, [1, 2], True, None)
    two = torch.randint(0, 2, (B, H, Wd))
    two[1, 2, 3] = 255
    emit('absent_present', 'probas', probas, two, 'present', False, 255)
    emit('absent_all', 'probas', probas, two, 'all', False, 255)
    logits = torch.randn(B, H, Wd) * 2
    mask = torch.randint(0, 2, (B, H, Wd))
    mask[0, 0, 1] = mask[0, 3, 3] = mask[1, 4, 0] = 255
    emit('hinge_image', 'hinge', logits, mask, [1], True, 255)
    emit('hinge_batch', 'hinge', logits, mask, [1], False, 255)
    logits3 = torch.randn(3, H, Wd) * 2
    mask3 = torch.randint(0, 2, (3, H, Wd))
    mask3[1] = 255
    emit('hinge_allvoid', 'hinge', logits3, mask3, [1], True, 255)
    sig = torch.sigmoid(torch.randn(B, H, Wd) * 2)
    emit('sigmoid', 'probas', sig, mask, [1], False, 255)


if __name__ == '__main__':
    main()
