"""HIP-event timing of the label-map cross-entropy and OHEM (ssseg_ce_labels_*, ssseg_ohem_labels_*,
csrc/seglosses.hip) next to the dense ones (ssseg_ce_*, ssseg_ohem_*: unchanged code, the yardstick) on the same
logits, in one process.  Each loss is one captured graph of its forward + backward (the way a training step runs
them); a window is `--reps` replays between one pair of events; five windows per loss, interleaved round by round, and
the median window counts.  The spread of a loss is (max - min) / median of its five windows: the
dense windows' own spread is what a difference has to exceed.

The sparse target is the uint8 argmax of the dense one-hot target (nothing void: the same arithmetic on every pixel);
`void` rows repeat the sparse losses with a share --void of the pixels set to 255.
Algorithmic bytes, forward + backward: dense CE 5 * B*C*HW*4 (logits and target read twice, gradient written once);
sparse CE 3 * B*C*HW*4 + 2 * B*HW (the label map instead of the target).

    python tools/bench_sparse_ce.py [--shape 16x19x512] > profiles/sparse_ce_kernels.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd')
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402


def captured(fn, x):
    """one graph of loss = fn(x); loss.backward()"""
    xr = x.detach().requires_grad_(True)

    def step():
        xr.grad = None
        fn(xr).backward()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g, xr


def window(g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--shape', default='16x19x512')
    ap.add_argument('--void', type=float, default=0.05)
    ap.add_argument('--thresh', type=float, default=0.7)
    ap.add_argument('--min-kept', type=int, default=100000)
    a = ap.parse_args()
    from ssseg import ops
    dev = torch.device('cuda', 0)
    B, C, S = (int(v) for v in a.shape.split('x'))
    HW = S * S
    g = torch.Generator(device=dev).manual_seed(C)
    x = 2 * torch.randn(B, C, S, S, device=dev, generator=g)
    y = torch.randint(0, C, (B, S, S), device=dev, generator=g)
    t = torch.nn.functional.one_hot(y, C).permute(0, 3, 1, 2).float().contiguous()
    y8 = y.to(torch.uint8)
    yv = y8.clone()
    yv[torch.rand(B, S, S, device=dev, generator=g) < a.void] = 255
    full = B * C * HW * 4
    losses = {
        'ce_dense': (5 * full, lambda v: ops.dense_cross_entropy(v, t, 'mean')),
        'ce_sparse': (3 * full + 2 * B * HW, lambda v: ops.cross_entropy_labels(v, y8)),
        'ce_sparse_void': (3 * full + 2 * B * HW, lambda v: ops.cross_entropy_labels(v, yv)),
        'ohem_dense': (None, lambda v: ops.ohem_cross_entropy(v, t, a.thresh, a.min_kept)),
        'ohem_sparse': (None, lambda v: ops.ohem_cross_entropy_labels(v, y8, a.thresh, a.min_kept)),
        'ohem_sparse_void': (None, lambda v: ops.ohem_cross_entropy_labels(v, yv, a.thresh, a.min_kept)),
    }
    graphs = {k: captured(fn, x) for k, (_, fn) in losses.items()}
    for gr, _ in graphs.values():      # warm every graph before the first window
        window(gr, 5)
    ms = {k: [] for k in losses}
    for _ in range(a.windows):
        for k, (gr, _) in graphs.items():
            ms[k].append(window(gr, a.reps))
    torch.cuda.synchronize()
    rows = {}
    for k, w in ms.items():
        s = sorted(w)
        med = s[len(s) // 2]
        rows[k] = dict(loss=k, B=B, C=C, HW=HW, reps=a.reps, windows_ms=[round(v, 4) for v in w],
                       ms_median=round(med, 4), spread=round((s[-1] - s[0]) / med, 4))
        if losses[k][0] is not None:
            rows[k].update(MB=round(losses[k][0] / 1e6, 1), GBps=round(losses[k][0] / med / 1e6, 1))
        print(json.dumps(rows[k]), flush=True)
    # the gradients of the no-void pairs are the same bits (tests/test_sparse_losses.py asserts it at small shapes)
    same = {p: bool(torch.equal(graphs[p + '_dense'][1].grad, graphs[p + '_sparse'][1].grad)) for p in ('ce', 'ohem')}
    for p in ('ce', 'ohem'):
        d, s = rows[p + '_dense'], rows[p + '_sparse']
        print(json.dumps({'pair': p, 'dense_ms': d['ms_median'], 'sparse_ms': s['ms_median'],
                          'sparse_over_dense': round(s['ms_median'] / d['ms_median'], 4), 'dense_spread': d['spread'],
                          'not_slower': bool(s['ms_median'] <= d['ms_median'] * (1 + d['spread'])),
                          'gradients_bitwise_equal': same[p]}), flush=True)


if __name__ == '__main__':
    main()
