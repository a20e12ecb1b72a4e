"""HIP-event timing of the ClassMix / CutMix mask kernels (csrc/mixmask.hip) from one process: 10 warm-up launches,
the median of `--reps` launches each timed on its own pair of events, two rounds over the same buffers (the
round-to-round spread of the medians).

Per shape BxCxS (S x S pixels):
  classmix_mask    memset + label + select + write (the whole ClassMix mask, as the step launches it);
  softmax_fwd      ssseg_consistency_sm_fwd on the same shape: the same register-row read pattern over two tensors,
                   the yardstick of the label kernel's GB/s;
  cutmix_mask      the CutMix mask;
  cowmix_mask      the CowMix mask at the same B, H, W (sigma 16, the middle of C2's range);
  draws            ssseg_mixmask_draw_dev for the keys.
The entry point launches the three ClassMix kernels back to back; their separate times come from a kernel trace of
this script (rocprofv3 --kernel-trace --stats -- python tools/bench_mixmask.py), DESIGN 14.

Algorithmic bytes: label reads B*C*HW*4 and writes B*HW; the whole ClassMix mask adds a B*HW read and a B*HW*4 write;
CutMix writes B*HW*4; softmax_fwd reads 2*B*C*HW*4.

    python tools/bench_mixmask.py [--reps 30] > profiles/mixmask_kernels.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd')
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[int(len(ms) * 0.9)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--shapes', default='16x19x512,16x2x512')
    a = ap.parse_args()
    from ssseg import native as N
    dev = torch.device('cuda', 0)
    for spec in a.shapes.split(','):
        B, C, S = (int(v) for v in spec.split('x'))
        HW = S * S
        g = torch.Generator(device=dev).manual_seed(C)
        t = 3 * torch.randn(B, C, S, S, device=dev, generator=g)
        s = torch.randn(B, C, S, S, device=dev, generator=g)
        keys = torch.randint(0, 2 ** 31, (B, C), device=dev, generator=g).to(torch.int32)
        params = torch.rand(B, 4, device=dev, generator=g)
        noise = torch.randn(B, S, S, device=dev, generator=g)
        sigma = torch.full((B,), 16.0, device=dev)
        prop = torch.full((B,), 0.5, device=dev)
        mask = torch.empty(B, 1, S, S, device=dev)
        out = torch.empty(3, device=dev)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        nb_red = N.lib().ssseg_reduce_workspace_bytes(B * HW)
        ws_red = N.workspace(nb_red, dev)
        nb_cm = N.lib().ssseg_classmix_workspace_bytes(B, S, S)
        ws_cm = N.workspace(nb_cm, dev)
        nb_cow = N.lib().ssseg_cowmix_workspace_bytes(B, S, S)
        ws_cow = N.workspace(nb_cow, dev)
        st, p, strides = N.stream(), N.dev_ptr, N.strides4(t)
        kernels = {
            'softmax_fwd': (2 * B * C * HW * 4, lambda: N.call('ssseg_consistency_sm_fwd', p(s), p(t), None, B, C, HW,
                                                               0.6, p(out), p(ws_red), nb_red, st)),
            'classmix_mask': (B * C * HW * 4 + B * HW * 6, lambda: N.call(
                'ssseg_classmix_mask', p(t), strides, N.F32, p(keys), B, C, S, S, p(mask), None, None, p(ws_cm), nb_cm,
                st)),
            'cutmix_mask': (B * HW * 4, lambda: N.call('ssseg_cutmix_mask', p(params), B, S, S, 0.45, 0.55, p(mask),
                                                       None, st)),
            'cowmix_mask': (6 * B * HW * 4, lambda: N.call('ssseg_cowmix_mask', p(noise), p(sigma), p(prop), B, S, S,
                                                           p(mask), None, None, p(ws_cow), nb_cow, st)),
            'draws': (B * C * 4, lambda: N.call('ssseg_mixmask_draw_dev', p(keys), None, B, C, 1234, p(ctr), st)),
        }
        for round_ in range(2):
            for name, (nbytes, fn) in kernels.items():
                med, lo, p90 = timed(fn, a.reps)
                print(json.dumps({'kernel': name, 'B': B, 'C': C, 'HW': HW, 'round': round_, 'reps': a.reps,
                                  'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_p90': round(p90, 4),
                                  'MB': round(nbytes / 1e6, 1), 'GBps': round(nbytes / med / 1e6, 1)}),
                      flush=True)
        del s, t, noise, mask
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
