"""HIP-event timing of the self-adaptive threshold update (ssseg_adaptive_thr_update, csrc/adaptive_thr.hip) and of the
pseudo-label cross-entropy with a threshold vector (ssseg_consistency_ce_cls_fwd / _bwd, csrc/multiclass.hip) next to
the unchanged scalar pair ssseg_consistency_ce_fwd / _bwd on the same buffers, from one process: 10 warm-up launches,
the median of `--reps` launches each timed on its own pair of events, two rounds over the same buffers (the
round-to-round spread of the scalar pair's medians is what a difference has to exceed).

Per shape BxCxS (S x S pixels):
  thr_update                    one update (the pass over t and the final block);
  ce_fwd_* / ce_bwd_*           the scalar pair (the yardstick: unchanged code), weighting 'pixel' and 'batch';
  ce_cls_fwd_* / ce_cls_bwd_*   the pair with the threshold vector (every entry --thr: the same decisions).
Algorithmic bytes: the update reads B*C*HW*4; a forward reads 2*B*C*HW*4, a backward reads that and writes B*C*HW*4.

    python tools/bench_adaptive_thr.py [--reps 30] > profiles/adaptive_thr_kernels.jsonl
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
    ap.add_argument('--momentum', type=float, default=0.999)
    ap.add_argument('--only', default='', help='comma-separated kernel-name prefixes (default: all)')
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
        out4 = {k: torch.empty(4, device=dev) for k in ((0, False), (1, False), (0, True), (1, True))}
        gout = torch.ones(1, device=dev)
        thr_c = torch.full((C,), a.thr, device=dev)
        state = torch.tensor([1.0 / C] * (C + 1) + [0.0] * (C + 2), dtype=torch.float64, device=dev)
        thr_out = torch.empty(C, device=dev)
        nb_ce = N.lib().ssseg_consistency_ce_workspace_bytes(B * HW)
        ws_ce = N.workspace(nb_ce, dev)
        nb_at = N.lib().ssseg_adaptive_thr_workspace_bytes(C)
        ws_at = N.workspace(nb_at, dev)
        st, p = N.stream(), N.dev_ptr
        one, fwd_bytes, bwd_bytes = B * C * HW * 4, 2 * B * C * HW * 4, 3 * B * C * HW * 4

        def fwd(wt, cls):
            name, th = ('ssseg_consistency_ce_cls_fwd', p(thr_c)) if cls else ('ssseg_consistency_ce_fwd', a.thr)
            return lambda: N.call(name, p(s), p(t), None, B, C, HW, th, wt, p(out4[wt, cls]), p(ws_ce), nb_ce, st)

        def bwd(wt, cls):
            name, th = ('ssseg_consistency_ce_cls_bwd', p(thr_c)) if cls else ('ssseg_consistency_ce_bwd', a.thr)
            return lambda: N.call(name, p(s), p(t), None, B, C, HW, th, wt, p(out4[wt, cls]), p(gout), p(gs), st)
        kernels = {'thr_update': (one, lambda: N.call('ssseg_adaptive_thr_update', p(t), B, C, HW, a.momentum, p(state),
                                                      p(thr_out), p(ws_at), nb_at, st))}
        for wt, wname in ((0, 'pixel'), (1, 'batch')):   # every forward runs before the backward that reads its sums
            kernels[f'ce_fwd_{wname}'] = (fwd_bytes, fwd(wt, False))
            kernels[f'ce_cls_fwd_{wname}'] = (fwd_bytes, fwd(wt, True))
        for wt, wname in ((0, 'pixel'), (1, 'batch')):
            kernels[f'ce_bwd_{wname}'] = (bwd_bytes, bwd(wt, False))
            kernels[f'ce_cls_bwd_{wname}'] = (bwd_bytes, bwd(wt, True))
        only = tuple(filter(None, a.only.split(',')))
        for round_ in range(2):
            for name, (nbytes, fn) in kernels.items():
                if only and not name.startswith(only):
                    continue
                med, lo, p90 = timed(fn, a.reps)
                print(json.dumps({'kernel': name, 'B': B, 'C': C, 'HW': HW, 'round': round_, 'reps': a.reps,
                                  'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_p90': round(p90, 4),
                                  'MB': round(nbytes / 1e6, 1), 'GBps': round(nbytes / med / 1e6, 1)}),
                      flush=True)
        torch.cuda.synchronize()
        print(json.dumps({'shape': spec, 'thr': a.thr, 'momentum': a.momentum, 'updates': int(state[C + 1]),
                          'tau': float(state[0]), 'thr_c_min_max': [float(thr_out.min()), float(thr_out.max())],
                          'out4': {f'{"cls" if c else "scalar"}_{w}': v.tolist() for (w, c), v in out4.items()}}),
              flush=True)
        del s, t, gs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
