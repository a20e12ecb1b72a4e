"""Time of one optimizer step per fused mode at C2's parameter count (the UNet-R50 arena), one process.

    python tools/optim_step_time.py [--reps 600] [--out profiles/optim_step_time.json]

Per mode (Adam, AdaMod, DiffGrad, DiffMod, Ranger) and for the existing fused SGD step, in the same run:
  update   prepare + update kernel (no clipping): microseconds and achieved GB/s from the bytes the mode must move
           (4 bytes x arena elements x the arenas it reads and writes; Ranger's slow buffer counts 2/k per step)
  clipped  the step the trainer issues (squared-norm pass + prepare + update, max_norm 5): the same, + one read of g
  torch    the same algorithm issued per tensor through torch ops (tests/optim_ref.py, after clip_grad_norm_)
The kernels are pure streaming, so the yardstick is the SGD kernel's achieved bandwidth in the same run
(`bw_vs_sgd`).  Timed with the fence-free HIP events of ssseg.nn.ProbeEvent around `reps` back-to-back steps.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import optimizers  # noqa: E402
from optim_ref import RefOptim  # noqa: E402
from ssseg import arena, optim  # noqa: E402
from ssseg.nn import ProbeEvent  # noqa: E402

# name -> (class, constructor keywords, arenas read + written by the update kernel, restatement's name)
MODES = {
    'sgd': (optim.SGD, dict(lr=1e-3, momentum=0.9, weight_decay=5e-4), 6, None),
    'adam': (optim.Adam, dict(lr=1e-3, weight_decay=5e-4), 7, 'adam'),
    'adamod': (optimizers.AdaMod, dict(lr=1e-3, weight_decay=5e-4), 9, 'adamod'),
    'diffgrad': (optimizers.DiffGrad, dict(lr=1e-3, weight_decay=5e-4), 9, 'diffgrad'),
    'diffmod': (optimizers.DiffMod, dict(lr=1e-3, weight_decay=5e-4), 11, 'diffmod'),
    'ranger': (optimizers.Ranger, dict(lr=1e-3, weight_decay=5e-4, k=6), 7 + 2 / 6, 'ranger'),
}


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = ProbeEvent(), ProbeEvent()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def c2_student(dev):
    from models import unet
    from models.adapters import ListOutput
    from models.encoders import resnet
    torch.manual_seed(0)
    return ListOutput(unet.UNet(2, resnet.resnet50_encoder(), max_width=128, train_upsampling=True)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=600)         # a multiple of Ranger's k; ~0.1 s per timed window
    ap.add_argument('--torch-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_step_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_step_time: needs the GPU (no timing without one)')
    dev = torch.device('cuda:0')
    model = c2_student(dev)
    ar = arena.attach(model)
    n = ar.numel
    start = ar.data.clone()
    grad = torch.randn(n, device=dev) * 1e-3
    rows = {}
    for name, (cls, kw, streams, ref) in MODES.items():
        ar.data.copy_(start)
        ar.grad.copy_(grad)
        opt = cls(model.parameters(), **kw)
        if name == 'sgd':
            opt.step()                      # the momentum buffer's first step
        row = {'arenas_moved': streams}
        for label, extra, kwargs in (('update', 0, {}), ('clipped', 1, dict(max_norm=5.0))):
            us = timeit(lambda: opt.step(**kwargs), a.reps)
            nbytes = 4.0 * n * (streams + extra)
            row[label] = {'us': round(us, 2), 'bytes': int(nbytes), 'GBps': round(nbytes / us * 1e-3, 1)}
        if ref is not None:
            params = list(model.parameters())
            r = RefOptim(ref, params, dtype=torch.float32, **kw)

            def torch_step():
                torch.nn.utils.clip_grad_norm_(params, 5.0)
                r.step([p.grad for p in params])
            row['torch'] = {'us': round(timeit(torch_step, a.torch_reps, warm=1), 1), 'tensors': len(params)}
            del r
        rows[name] = row
        del opt
        torch.cuda.empty_cache()
    sgd_bw = rows['sgd']['update']['GBps']
    for name, row in rows.items():
        row['bw_vs_sgd'] = round(row['update']['GBps'] / sgd_bw, 3)
    res = {'device': torch.cuda.get_device_name(0), 'arena_elements': n, 'reps': a.reps,
           'note': 'update = prepare + update kernel; clipped = + squared-norm pass (what train_step issues); '
                   'torch = clip_grad_norm_ + per-tensor torch ops; GBps from the bytes each mode must move',
           'modes': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    for name, row in rows.items():
        t = row.get('torch', {}).get('us')
        print(f"{name:9s} update {row['update']['us']:8.1f} us {row['update']['GBps']:7.1f} GB/s  "
              f"clipped {row['clipped']['us']:8.1f} us {row['clipped']['GBps']:7.1f} GB/s  "
              f"x{row['bw_vs_sgd']:.2f} of SGD's bandwidth" + (f"  per-tensor torch {t:9.1f} us" if t else ''))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
