"""Post-training int8 export -- the reference's inference.py (best checkpoint -> conv+BN fusion -> calibration on 200
unlabelled images -> torch.quantization prepare / convert on fbgemm -> model_quantized.ts) on the device's integer
matrix pipe, without cv2 windows, TorchScript and fbgemm:

    inference.py CONFIG --checkpoint PATH --out FILE [--images DIR ...] [--weights ema|student]
        [--calib-images 200] [--batch-size N] [--rule measured|all]

The model is built from the config as distributed_trainer does and the checkpoint read by its dict keys (default
ema_state_dict, the teacher).  Calibration runs eval forwards over the first --calib-images images of the config's
unlabelled dataset (train['unsupervised_dataset']), or of the given directories read through
UnsupervisedImagesDataset with the validation-time transforms; every eligible conv observes max |input|
(ssseg.quant.calibrating).  quant.convert then derives the int8 weights and freezes the BN folds of the convs --rule
selects: 'measured' keeps the layer classes that measured slower in int8 in the 16-bit path (today every class of the
measured table, DESIGN.md 23: the file then carries the calibration only), 'all' converts every calibrated conv.  FILE
receives

    {'state_dict': the model's weights, 'quant': ssseg.quant.state_dict(model), 'meta': {...}}

which a server loads with model.load_state_dict(f['state_dict']); quant.load_state_dict(model, f['quant'],
rule=f['meta']['rule']); quant.QuantizedModel(model).  One JSON line reports, over the config's validation set, the share of pixels on which
the 16-bit and the int8 predictions agree (argmax) and both models' mIoU.
"""
import argparse
import json
import os
import sys

WEIGHT_KEYS = {'ema': 'ema_state_dict', 'student': 'state_dict'}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Calibrate a trained model, convert it to int8 and save it.')
    p.add_argument('config')
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--out', required=True, metavar='FILE')
    p.add_argument('--images', nargs='+', metavar='DIR', help='calibration images (default: the config\'s '
                                                              'unlabelled dataset)')
    p.add_argument('--weights', choices=sorted(WEIGHT_KEYS), default='ema')
    p.add_argument('--calib-images', type=int, default=200)
    p.add_argument('--rule', choices=('measured', 'all'), default='measured',
                   help="which calibrated convs become int8: those of the layer classes that measured faster in int8 "
                        "(ssseg.quant.worth_int8; the default) or all of them")
    p.add_argument('--batch-size', type=int)
    a = p.parse_args(argv)
    if a.calib_images < 1 or (a.batch_size is not None and a.batch_size < 1):
        p.error('--calib-images and --batch-size must be positive')
    return a


def _images(batch):
    return batch['image'] if isinstance(batch, dict) else batch


def calibration_loader(cfg, args, batch_size):
    import torch
    if args.images:
        from data.unsupervised_dataset import UnsupervisedImagesDataset
        from get_active_learning_partition import validation_transforms
        pool = UnsupervisedImagesDataset(args.images, validation_transforms(cfg))
        pool.filenames.sort()
    else:
        pool = cfg['train']['unsupervised_dataset']()
    n = min(len(pool), args.calib_images)
    if n < 1:
        raise ValueError('inference.py: no calibration images')
    return torch.utils.data.DataLoader(torch.utils.data.Subset(pool, range(n)), batch_size=batch_size, shuffle=False)


class Confusion:
    """running C x C confusion matrix (rows label, columns prediction) on the device; void labels left out"""

    def __init__(self, ignore_label):
        self.ignore, self.total = ignore_label, None

    def update(self, pred, mask):
        import torch
        C = pred.shape[1]
        label = mask.long() if mask.dim() == 3 else mask.argmax(1)
        p = pred.argmax(1)
        if p.shape[-2:] != label.shape[-2:]:   # the argmax map, nearest-resized to the mask (train.validate's metric)
            p = torch.nn.functional.interpolate(p[:, None].float(), size=label.shape[-2:], mode='nearest')[:, 0].long()
        keep = (label >= 0) & (label < C)
        if self.ignore is not None:
            keep &= label != self.ignore
        m = torch.bincount(label[keep] * C + p[keep], minlength=C * C).view(C, C)
        self.total = m if self.total is None else self.total + m
        return p, keep

    def miou(self):
        t = self.total.double()
        inter = t.diagonal()
        union = t.sum(0) + t.sum(1) - inter
        ious = [float(i / u) if u else 1.0 for i, u in zip(inter, union)]
        return 100.0 * sum(ious) / len(ious)


def compare(model, qmodel, loader, device, ignore_label):
    """-> (argmax agreement in [0, 1], mIoU of the 16-bit model, mIoU of the int8 model) over the loader"""
    import torch
    ca, cb = Confusion(ignore_label), Confusion(ignore_label)
    same = torch.zeros((), dtype=torch.int64, device=device)
    count = 0
    with torch.no_grad():
        for sample in loader:
            image, mask = sample['image'].to(device), sample['semantic_mask'].to(device)
            pa, _ = ca.update(model(image)[1][-1], mask)
            pb, _ = cb.update(qmodel(image)[1][-1], mask)
            same += (pa == pb).sum()
            count += pa.numel()
    return float(same) / max(count, 1), ca.miou(), cb.miou()


def main(argv=None):
    args = parse_args(argv)
    import torch

    import config
    from ssseg import nn as snn
    from ssseg import quant

    cfg = config.fromfile(args.config)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    snn.set_compute_dtype({'fp32': torch.float32, 'fp16': torch.float16}.get(cfg['common'].get('compute_dtype'),
                                                                             torch.bfloat16))
    model = cfg['model']['model_fn']().to(device)
    ck = torch.load(args.checkpoint, map_location='cpu')
    key = WEIGHT_KEYS[args.weights]
    if key not in ck:
        raise KeyError(f'{args.checkpoint}: no {key!r} (keys: {sorted(ck)})')
    model.load_state_dict(ck[key], strict=False)
    model.eval()
    bs = args.batch_size or int((cfg.get('val') or {}).get('batch_size_per_worker', 8))

    quant.prepare(model)
    seen = 0
    with quant.calibrating(model):
        for batch in calibration_loader(cfg, args, bs):
            images = _images(batch).to(device)
            model(images)
            seen += int(images.shape[0])
    quant.convert(model, rule=args.rule)
    rows = quant.summary(model)
    n_int8 = sum(1 for r in rows if r['int8'])

    qmodel = quant.QuantizedModel(model)
    val = torch.utils.data.DataLoader(cfg['val']['dataset'](), batch_size=bs, shuffle=False)
    agreement, miou_a, miou_b = compare(model, qmodel, val, device, cfg['train'].get('ignore_label'))
    report = {'config': args.config, 'checkpoint': args.checkpoint, 'weights': args.weights,
              'calibration_images': seen, 'rule': args.rule, 'convs': len(rows), 'convs_int8': n_int8,
              'argmax_agreement': agreement, 'miou_16bit': miou_a, 'miou_int8': miou_b}
    torch.save({'state_dict': model.state_dict(), 'quant': quant.state_dict(model), 'meta': report}, args.out)
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
