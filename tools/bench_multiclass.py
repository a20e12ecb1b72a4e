"""HIP-event timing of the softmax consistency kernels (csrc/multiclass.hip) beside the two-class sigmoid kernels
(csrc/eltwise.hip) from the same run: warm-up, `--reps` launches each timed on its own pair of events, the median and
the spread, and the algorithmic bytes over the median.

Algorithmic bytes: forward reads s and t (2 * B*C*HW * 4), backward reads both and writes gs (3 * B*C*HW * 4).

    python tools/bench_multiclass.py [--reps 50] > profiles/multiclass_kernels.jsonl
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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--shapes', default='16x19x512,16x2x512,16x64x256')
    a = ap.parse_args()
    from ssseg import native as N
    dev = torch.device('cuda', 0)
    thr = 0.6
    for spec in a.shapes.split(','):
        B, C, S = (int(v) for v in spec.split('x'))
        HW = S * S
        g = torch.Generator(device=dev).manual_seed(C)
        s = torch.randn(B, C, HW, device=dev, generator=g)
        t = 3 * torch.randn(B, C, HW, device=dev, generator=g)
        gs = torch.empty_like(s)
        out = torch.empty(3, device=dev)
        gout = torch.ones(1, device=dev)
        nb = N.lib().ssseg_reduce_workspace_bytes(B * HW)
        ws = N.workspace(nb, dev)
        st = N.stream()
        p = N.dev_ptr
        kernels = {
            'softmax_fwd': (2, lambda: N.call('ssseg_consistency_sm_fwd', p(s), p(t), None, B, C, HW, thr, p(out),
                                              p(ws), nb, st)),
            'softmax_bwd': (3, lambda: N.call('ssseg_consistency_sm_bwd', p(s), p(t), None, B, C, HW, thr, p(out),
                                              p(gout), p(gs), st)),
        }
        if C == 2:   # the yardstick: the two-class sigmoid kernels at equal bytes
            kernels['sigmoid_fwd'] = (2, lambda: N.call('ssseg_consistency_fwd', p(s), p(t), B, C, HW, thr, p(out),
                                                        p(ws), nb, st))
            kernels['sigmoid_bwd'] = (3, lambda: N.call('ssseg_consistency_bwd', p(s), p(t), B, C, HW, thr, p(out),
                                                        p(gout), p(gs), st))
        for round_ in range(2):   # two rounds over the same buffers: the run-to-run spread of the medians
            for name, (passes, fn) in kernels.items():
                med, lo, p90 = timed(fn, a.reps)
                nbytes = passes * B * C * HW * 4
                print(json.dumps({'kernel': name, 'B': B, 'C': C, 'HW': HW, 'round': round_, 'reps': a.reps,
                                  'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_p90': round(p90, 4),
                                  'MB': round(nbytes / 1e6, 1), 'GBps': round(nbytes / med / 1e6, 1),
                                  'confident_fraction': round(float(out[1]), 4)}), flush=True)
        del s, t, gs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
