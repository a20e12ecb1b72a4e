"""HIP-event timing of the pseudo-label consistency kernels (ssseg_consistency_ce_fwd / _bwd, csrc/multiclass.hip) next
to the softmax-MSE pair ssseg_consistency_sm_fwd / _bwd on the same buffers, from one process: 10 warm-up launches, the
median of `--reps` launches each timed on its own pair of events, two rounds over the same buffers (the round-to-round
spread of the medians; the yardstick's own spread is what a difference has to exceed).

Per shape BxCxS (S x S pixels), weighting 'pixel' and 'batch':
  sm_fwd / sm_bwd          the MSE pair (the yardstick: unchanged code);
  ce_fwd_* / ce_bwd_*      the CE pair.
Algorithmic bytes: a forward reads 2*B*C*HW*4, a backward reads that and writes B*C*HW*4 (the weight map is NULL).

    python tools/bench_pseudo_ce.py [--reps 30] > profiles/pseudo_ce_kernels.jsonl
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
    ap.add_argument('--thr', type=float, default=0.6)
    a = ap.parse_args()
    from ssseg import native as N
    dev = torch.device('cuda', 0)
    for spec in a.shapes.split(','):
        B, C, S = (int(v) for v in spec.split('x'))
        HW = S * S
        g = torch.Generator(device=dev).manual_seed(C)
        t = 3 * torch.randn(B, C, S, S, device=dev, generator=g)
        s = torch.randn(B, C, S, S, device=dev, generator=g)
        gs = torch.empty_like(s)
        out3 = torch.empty(3, device=dev)
        out4 = {0: torch.empty(4, device=dev), 1: torch.empty(4, device=dev)}
        gout = torch.ones(1, device=dev)
        nb_red = N.lib().ssseg_reduce_workspace_bytes(B * HW)
        ws_red = N.workspace(nb_red, dev)
        nb_ce = N.lib().ssseg_consistency_ce_workspace_bytes(B * HW)
        ws_ce = N.workspace(nb_ce, dev)
        st, p = N.stream(), N.dev_ptr
        fwd_bytes, bwd_bytes = 2 * B * C * HW * 4, 3 * B * C * HW * 4

        def ce_fwd(wt):
            return lambda: N.call('ssseg_consistency_ce_fwd', p(s), p(t), None, B, C, HW, a.thr, wt, p(out4[wt]),
                                  p(ws_ce), nb_ce, st)

        def ce_bwd(wt):
            return lambda: N.call('ssseg_consistency_ce_bwd', p(s), p(t), None, B, C, HW, a.thr, wt, p(out4[wt]),
                                  p(gout), p(gs), st)
        kernels = {
            'sm_fwd': (fwd_bytes, lambda: N.call('ssseg_consistency_sm_fwd', p(s), p(t), None, B, C, HW, a.thr, p(out3),
                                                 p(ws_red), nb_red, st)),
            'ce_fwd_pixel': (fwd_bytes, ce_fwd(0)),
            'ce_fwd_batch': (fwd_bytes, ce_fwd(1)),
            'sm_bwd': (bwd_bytes, lambda: N.call('ssseg_consistency_sm_bwd', p(s), p(t), None, B, C, HW, a.thr, p(out3),
                                                 p(gout), p(gs), st)),
            'ce_bwd_pixel': (bwd_bytes, ce_bwd(0)),
            'ce_bwd_batch': (bwd_bytes, ce_bwd(1)),
        }
        for round_ in range(2):
            for name, (nbytes, fn) in kernels.items():   # every forward runs before the backward that reads its sums
                med, lo, p90 = timed(fn, a.reps)
                print(json.dumps({'kernel': name, 'B': B, 'C': C, 'HW': HW, 'round': round_, 'reps': a.reps,
                                  'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_p90': round(p90, 4),
                                  'MB': round(nbytes / 1e6, 1), 'GBps': round(nbytes / med / 1e6, 1)}),
                      flush=True)
        torch.cuda.synchronize()
        print(json.dumps({'shape': spec, 'thr': a.thr, 'sm_out3': out3.tolist(), 'ce_out4_pixel': out4[0].tolist(),
                          'ce_out4_batch': out4[1].tolist()}), flush=True)
        del s, t, gs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
