"""A/B of the int8 inference path (ssseg/quant.py, csrc/quant.hip) against the 16-bit eval forward, in one process with
the two modes interleaved window by window and timed with the fence-free probe events (ssseg.nn.ProbeEvent):

  layers    every distinct eligible conv geometry of the C2 eval forward (UNet-R50, 512^2, batch 16): the bf16
            `_ssseg_forward` (folded BN, residual, activation) against ssseg_quantize_i8 + ssseg_conv_i8_fwd, and the
            quantise pass alone;
  model     the whole-model eval forward in both modes;
  accuracy  (--accuracy) configs/c6_unet_r50_labelmap.py trained on its synthetic set for --train-steps supervised
            steps, the student calibrated on the unlabelled set and converted: bf16 against int8 mIoU and argmax
            agreement over the validation set.  Synthetic data only: a reported measurement, not a pass condition.

A window is one replay of `--reps` calls captured into a HIP graph (device time: issued from Python most of these layers
are bound by the host); the median of `--windows` windows counts; spread = (max - min) / median.

    python tools/quant_ab.py [--accuracy] > profiles/quant_ab.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd')
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402


def captured(fn, reps):
    """`reps` calls as one HIP graph: a Python-issued conv call costs ~40 us of host time, more than most of these
    layers take on the device, so the device time is that of the replay"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g


def timed(graph, reps):
    from ssseg import nn as snn
    a, b = snn.ProbeEvent(), snn.ProbeEvent()
    a.record()
    graph.replay()
    b.record()
    return a.elapsed_time(b) / reps


def median_spread(ms):
    s = sorted(ms)
    med = s[len(s) // 2]
    return round(med, 4), round((s[-1] - s[0]) / med, 3)


def interleaved(fns, reps, windows):
    """{name: (median ms per call, spread)} of the callables, one window (a replay of `reps` captured calls) of each
    per round"""
    graphs = {k: captured(fn, reps) for k, fn in fns.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(windows):
        for k, g in graphs.items():
            ms[k].append(timed(g, reps))
    torch.cuda.synchronize()
    return {k: median_spread(v) for k, v in ms.items()}


def c2_model(dev, classes=2):
    from models.adapters import ListOutput
    from models.encoders.resnet import resnet50_encoder
    from models.unet import UNet
    torch.manual_seed(0)
    return ListOutput(UNet(classes, resnet50_encoder(), max_width=128, norm_layer=torch.nn.BatchNorm2d,
                           train_upsampling=True)).to(dev).eval()


def bench_layers(model, image, reps, windows):
    from ssseg import native as N
    from ssseg import nn as snn
    from ssseg import quant
    # the launches of one quantised forward, by distinct geometry
    with quant.trace() as rows, quant.quantized(model):
        model(image)
    seen, out = set(), []
    for r in rows:
        conv, x = r['conv'], r['input']
        key = (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.dilation, tuple(x.shape),
               r['residual'] is not None, r['bn'] is not None)
        if key in seen:
            continue
        seen.add(key)
        rec = conv.__dict__['_ssseg_q']
        x = x.clone()
        res = r['residual'].clone() if r['residual'] is not None else None
        relu, bn = r['act'], r['bn']
        n, cp, H, W = x.shape
        ldq = snn.rup(conv.in_channels, 16)
        q = torch.empty((n, H, W, ldq), dtype=torch.int8, device=x.device)

        def bf16():
            with torch.no_grad():
                conv._ssseg_forward(x, relu, bn=bn, residual=res)

        def int8():
            with quant.quantized(model):
                conv._ssseg_forward(x, relu, bn=bn, residual=res)

        def quantise_only():
            N.call('ssseg_quantize_i8', N.dev_ptr(x), n * H * W, conv.in_channels, cp, N.dt_code(x),
                   N.dev_ptr(rec.slot), N.dev_ptr(q), ldq, N.stream())

        t = interleaved({'bf16': bf16, 'int8': int8, 'quantise': quantise_only}, reps, windows)
        R, S = conv.kernel_size
        OH, OW = conv._out_hw(H, W)
        gflop = 2.0 * n * OH * OW * conv.out_channels * conv.in_channels * R * S / 1e9
        row = dict(name='layer', conv=rec.name, cin=conv.in_channels, cout=conv.out_channels, taps=[R, S],
                   stride=conv.stride[0], input=[n, H, W], contraction=R * S * conv.in_channels,
                   residual=res is not None, bf16_ms=t['bf16'][0], int8_ms=t['int8'][0], quantise_ms=t['quantise'][0],
                   spread=[t['bf16'][1], t['int8'][1]], int8_over_bf16=round(t['int8'][0] / t['bf16'][0], 3),
                   bf16_tflops=round(gflop / t['bf16'][0], 1), int8_tops=round(gflop / t['int8'][0], 1))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_model(model, image, reps, windows):
    from ssseg import quant
    qm = quant.QuantizedModel(model)

    def bf16():
        with torch.no_grad():
            model(image)

    t = interleaved({'bf16': bf16, 'int8': lambda: qm(image)}, reps, windows)
    n_int8 = sum(1 for r in quant.summary(model) if r['int8'])
    row = dict(name='model_eval_forward', model='UNet-R50', input=list(image.shape), convs_int8=n_int8,
               bf16_ms=t['bf16'][0], int8_ms=t['int8'][0], spread=[t['bf16'][1], t['int8'][1]],
               int8_over_bf16=round(t['int8'][0] / t['bf16'][0], 3))
    print(json.dumps(row), flush=True)
    return row


def calibrate(model, batches):
    from ssseg import quant
    quant.prepare(model)
    with quant.calibrating(model):
        for x in batches:
            model(x)
    quant.convert(model, rule='all')   # every eligible conv: the table is what the measured rule is chosen from


def accuracy(dev, steps, calib_images):
    """train C6-labelmap on its synthetic set (train.train_step, as the trainer runs it), then compare the teacher's
    bf16 and int8 predictions on the validation set"""
    import config
    import inference
    import mean_teacher
    import train
    from ssseg import arena
    from ssseg import nn as snn
    from ssseg import optim as soptim
    from ssseg import quant
    cfg = config.fromfile(os.path.join(PKG, 'configs/c6_unet_r50_labelmap.py'))
    snn.set_compute_dtype(torch.bfloat16)
    tc = cfg['train']
    tc['print_freq'] = 10 ** 9
    # supervised steps only: from a random init on this set the teacher never passes the config's 0.97 confidence in a
    # few hundred steps, and a consistency loss without a confident pixel is the reference's own 0/0 (NaN weights)
    tc['use_semi_supervised'] = False
    torch.manual_seed(0)
    student = cfg['model']['model_fn']().to(dev)
    teacher = cfg['model']['model_fn']().to(dev)
    teacher.load_state_dict(student.state_dict())
    mean_teacher.detach_model_parameters(teacher)
    teacher.eval()
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = soptim.from_config(tc['optimizer'], [p for p in student.parameters() if p.requires_grad])
    b = tc['batch_size_per_worker']
    lab, unl = tc['dataset'](), tc['unsupervised_dataset']()
    nlab, nunl = min(len(lab), 4 * b), min(len(unl), 8 * b)
    imgs = torch.stack([lab[i]['image'] for i in range(nlab)]).to(dev)
    masks = torch.stack([lab[i]['semantic_mask'] for i in range(nlab)]).to(dev)
    pool = torch.stack([unl[i]['image'] for i in range(nunl)]).to(dev)
    student.train()
    opt.zero_grad()
    losses = []
    for step in range(steps):
        i, j = (step * b) % nlab, (2 * step * b) % nunl
        k = (j + b) % nunl
        c, u, _ = train.train_step(student, teacher, opt, imgs[i:i + b], masks[i:i + b], pool[j:j + b], pool[k:k + b],
                                   30, step, cfg)
        if step % 50 == 0 or step == steps - 1:
            losses.append((step, round(float(c), 4), round(float(u), 4) if u is not None else None))
    torch.cuda.synchronize()
    student.eval()
    snn.invalidate_packed(student)
    calibrate(student, [pool[i:i + b] for i in range(0, min(calib_images, nunl), b)])
    val = torch.utils.data.DataLoader(cfg['val']['dataset'](), batch_size=b, shuffle=False)
    agree, miou_a, miou_b = inference.compare(student, quant.QuantizedModel(student), val, dev, tc.get('ignore_label'))
    row = dict(name='accuracy_synthetic', config='c6_unet_r50_labelmap', train_steps=steps, losses=losses,
               calibration_images=min(calib_images, nunl), argmax_agreement=round(agree, 5),
               miou_bf16=round(miou_a, 3), miou_int8=round(miou_b, 3),
               note='synthetic set: the images are noise independent of the labels; real-data accuracy is unmeasured')
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--accuracy', action='store_true')
    ap.add_argument('--no-timing', action='store_true', help='with --accuracy: the accuracy part alone')
    ap.add_argument('--train-steps', type=int, default=200)
    ap.add_argument('--calib-images', type=int, default=64)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.bfloat16)
    if not a.no_timing:
        model = c2_model(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        image = torch.rand(a.batch, 3, a.size, a.size, device=dev, generator=g)
        calibrate(model, [image, torch.rand(a.batch, 3, a.size, a.size, device=dev, generator=g)])
        bench_layers(model, image, a.reps, a.windows)
        bench_model(model, image, max(a.reps // 2, 2), a.windows)
        del model, image
        torch.cuda.empty_cache()
    if a.accuracy:
        accuracy(dev, a.train_steps, a.calib_images)


if __name__ == '__main__':
    main()
