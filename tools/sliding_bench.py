"""HIP-event timing of sliding-window evaluation (csrc/sliding.hip, ssseg/sliding.py).

Workload: C = 19, one 1024 x 2048 image, crop 512, stride 341 (3 x 6 windows), window_batch 8, softmax, uniform
weights, flip off (18 windows, 3 batches) and on (36 windows, 5 batches).  Per image:
  (a) `fused`: the ssseg_window_accumulate calls of every batch, against their algorithmic bytes -- the logits of the
      real windows read once, plus the accumulator and weight-sum pixels each call covers read and written once;
  (b) `composed`: the same fusion from what existed before: ops.interpolate_bilinear to the crop size (skipped where
      the logits are at the crop's resolution already), ops.prob_onehot (softmax), and one slice add per window;
  (c) `--end-to-end`: ms per image of UNet-R50 in bf16, SlidingWindowInference against the single whole-image forward
      followed by ops.prob_onehot.
(a) and (b) run on the same random logits at the crop's resolution and at half of it (a model that emits its logits
at stride 2), their windows interleaved round by round: the median of `--windows` windows of `--reps` images counts,
spread = (max - min) / median.  The fused sum has to be at least as fast as the composed one (exit status 1 if not)
and to agree with it to fp32 rounding; everything else is reported.

    python tools/sliding_bench.py --end-to-end > profiles/sliding_window.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd')
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
C, SIZE, CROP, STRIDE, WB = 19, (1024, 2048), (512, 512), 341, 8


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(name, ms, **extra):
    s = sorted(ms)
    med = s[len(s) // 2]
    row = dict(name=name, windows_ms=[round(v, 4) for v in ms], ms_median=round(med, 4),
               spread=round((s[-1] - s[0]) / med, 4), **extra)
    return med, row


def covered_pixels(rows):
    """accumulator pixels that at least one real window of the call covers"""
    m = torch.zeros(SIZE, dtype=torch.bool)
    for b, y0, x0, f in rows:
        if not f & 2:
            m[y0:y0 + CROP[0], x0:x0 + CROP[1]] = True
    return int(m.sum())


def bench_accumulate(flip, res, reps, windows, dev):
    from ssseg import ops, sliding
    runner = sliding.SlidingWindowInference(None, CROP, stride=STRIDE, flip=flip, window_batch=WB)
    rows = runner.windows(1, *SIZE)
    table, host = sliding.window_table(rows, dev)
    h, w = CROP[0] // res, CROP[1] // res
    g = torch.Generator(device=dev).manual_seed(res + 2 * flip)
    logits = [3 * torch.randn(WB, C, h, w, device=dev, generator=g) for _ in range(0, len(rows), WB)]
    acc = torch.zeros(1, C, *SIZE, device=dev)
    wsum = torch.zeros(1, *SIZE, device=dev)
    acc2, wsum2 = torch.zeros_like(acc), torch.zeros_like(wsum)

    def fused():
        for i, lg in enumerate(logits):
            k = i * WB
            sliding.window_accumulate(lg, table[k:k + WB], host[k:k + WB], CROP, acc, wsum, 'softmax', 'uniform')

    def composed():
        for i, lg in enumerate(logits):
            prob, _ = ops.prob_onehot(ops.interpolate_bilinear(lg, CROP, align_corners=False), 'softmax')
            for j, (b, y0, x0, f) in enumerate(rows[i * WB:(i + 1) * WB]):
                if f & 2:
                    continue
                acc2[b, :, y0:y0 + CROP[0], x0:x0 + CROP[1]] += prob[j].flip(-1) if f & 1 else prob[j]
                wsum2[b, y0:y0 + CROP[0], x0:x0 + CROP[1]] += 1

    # one image each from zero: the two sums agree to fp32 rounding (the same terms in the same order; the fused kernel
    # does not contract its products, the resize kernel is shared)
    fused()
    composed()
    torch.cuda.synchronize()
    diff = float((acc / wsum[:, None] - acc2 / wsum2[:, None]).abs().max())
    wdiff = float((wsum - wsum2).abs().max())
    for _ in range(2):
        fused()
        composed()
    torch.cuda.synchronize()
    ms = {'fused': [], 'composed': []}
    for _ in range(windows):
        ms['fused'].append(timed(fused, reps))
        ms['composed'].append(timed(composed, reps))
    real = [r for r in rows if not r[3] & 2]
    nbytes = len(real) * C * h * w * 4
    nbytes += sum(covered_pixels(rows[k:k + WB]) for k in range(0, len(rows), WB)) * (C + 1) * 4 * 2
    shape = dict(C=C, image=list(SIZE), crop=list(CROP), stride=STRIDE, window_batch=WB, flip=flip, logits_hw=[h, w],
                 windows=len(real), calls=len(logits), reps=reps)
    fm, frow = summary('window_accumulate', ms['fused'], **shape, algorithmic_MB=round(nbytes / 1e6, 1))
    frow.update(GBps=round(nbytes / fm / 1e6, 1), hbm_measured_share=round(nbytes / (fm * 1e-3) / HBM_MEASURED, 3),
                hbm_spec_share=round(nbytes / (fm * 1e-3) / HBM_SPEC, 3))
    cm, crow = summary('composed_resize_softmax_sliceadd', ms['composed'], **shape)
    print(json.dumps(frow), flush=True)
    print(json.dumps(crow), flush=True)
    ok = fm <= cm
    print(json.dumps(dict(name='fused_vs_composed', flip=flip, logits_hw=[h, w], fused_over_composed=round(fm / cm, 4),
                          fused_not_slower=bool(ok), max_abs_diff_mean=diff, max_abs_diff_wsum=wdiff)), flush=True)
    return ok


def bench_end_to_end(flip, reps, windows, dev):
    from models.adapters import ListOutput
    from models.encoders.resnet import resnet50_encoder
    from models.unet import UNet
    from ssseg import nn as snn
    from ssseg import ops, sliding
    snn.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = ListOutput(UNet(C, resnet50_encoder(), max_width=128, norm_layer=torch.nn.BatchNorm2d,
                            train_upsampling=True)).to(dev).eval()
    image = torch.rand(1, 3, *SIZE, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    runner = sliding.SlidingWindowInference(model, CROP, stride=STRIDE, flip=flip, activation='softmax',
                                            window_batch=WB)

    def whole():
        with torch.no_grad():
            _, maps = model(image)
            return ops.prob_onehot(ops.interpolate_bilinear(maps[-1].float(), SIZE, align_corners=False), 'softmax')[0]

    for fn in (lambda: runner(image), whole):          # every conv geometry tuned before the first window
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {'sliding': [], 'whole_image': []}
    for _ in range(windows):
        ms['sliding'].append(timed(lambda: runner(image), reps))
        ms['whole_image'].append(timed(whole, reps))
    shape = dict(model='UNet-R50 bf16', C=C, image=list(SIZE), crop=list(CROP), stride=STRIDE, window_batch=WB,
                 flip=flip, reps=reps)
    sm, srow = summary('end_to_end_sliding', ms['sliding'], **shape)
    wm, wrow = summary('end_to_end_whole_image', ms['whole_image'], **shape)
    print(json.dumps(srow), flush=True)
    print(json.dumps(wrow), flush=True)
    print(json.dumps(dict(name='sliding_over_whole_image', flip=flip, ratio=round(sm / wm, 4),
                          pixels_ratio=round(len(runner.windows(1, *SIZE)) * CROP[0] * CROP[1] / (SIZE[0] * SIZE[1]), 3))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--end-to-end', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    ok = True
    for flip in (False, True):
        for res in (1, 2):
            ok = bench_accumulate(flip, res, a.reps, a.windows, dev) and ok
    if a.end_to_end:
        for flip in (False, True):
            bench_end_to_end(flip, max(a.reps // 3, 2), a.windows, dev)
    if not ok:
        raise SystemExit('sliding_bench: the fused accumulate is slower than the composed path')


if __name__ == '__main__':
    main()
