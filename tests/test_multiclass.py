"""GPU: the multi-class kernels (csrc/multiclass.hip) through their public entry points -- the softmax consistency
loss, the C-class validation metrics, the C-class inference head -- and the training step, validation and inference
wrapper that use them, against the fp64 restatements of tests/multiclass_ref.py.

Bounds: the project's loss bounds, imported from test_hip_losses_ext.py (loss rtol 2e-5 atol 1e-7; gradient rtol 2e-4
atol 2e-8 at every element, exactly 0.0 wherever the fp64 gradient is 0); integer outputs bit for bit; the float
metrics rtol 1e-6 against fp64; the step against the oracle under the rules tests/test_bench_geometry.py applies to C1
(tests/parity.py).  The kernel's own thresholds: the 256-pixel tile (17*31 = 527 pixels per
sample: two full tiles and a partial one, a sample boundary inside a wavefront) and the channel buckets 2, 4, 8, 16,
32, 64 (C = 4, 5, 8, 9, 16, 17, 32, 33 sit on both sides of every edge).  Every test prints its figures before it
asserts.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_losses as E
import multiclass_ref as R
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu

THR = 0.7


def _maxabs(a):
    a = np.abs(np.asarray(a, np.float64)).reshape(-1)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else float('nan')


def close(a, ref, tol):
    return bool(np.allclose(a, ref, equal_nan=True, **tol))


def device_cons(s, t, thr, w, dev, gout=1.0):
    """-> (loss, cm mean, gradient of gout * loss) as numpy"""
    from ssseg import ops
    x = s.to(dev).requires_grad_(True)
    loss, cm = ops.consistency_loss_softmax(x, t.to(dev), thr, None if w is None else w.to(dev))
    assert not cm.requires_grad
    (loss * gout).backward()
    return loss.detach().cpu().numpy(), cm.detach().cpu().numpy(), x.grad.cpu().numpy()


def design(shape, seed, frac=0.6, scale=1.0):
    """student and teacher logits with every pixel's teacher confidence at least 1e-3 away from THR (asserted)"""
    g = torch.Generator().manual_seed(seed + 1000)
    s = (torch.randn(*shape, generator=g) * scale).contiguous()
    t, conf = R.confident_teacher(shape, THR, seed, frac=frac, scale=scale)
    p = torch.softmax(t.double(), 1).amax(1)
    assert float((p - THR).abs().min()) >= 1e-3 and torch.equal(p > THR, conf)
    return s, t, conf


def check_cons(name, s, t, conf, dev, w=None, gout=1.0):
    l64, cm64, cnt64, g64 = R.consistency_softmax_grad(s, t, THR, w, gout)
    loss, cm, grad = device_cons(s, t, THR, w, dev, gout)
    bad = ~np.isclose(grad, g64, equal_nan=True, **GRAD_TOL)
    print(f'{name} {tuple(s.shape)}: loss dev {loss!r} fp64 {l64!r} | cm {cm!r} fp64 {cm64!r} (count {cnt64!r}) | grad '
          f'dev-fp64 {_maxabs(grad - g64):.3e} of {_maxabs(g64):.3e}, {int(bad.sum())} of {bad.size} out of bound')
    assert loss.dtype == np.float32 and grad.shape == g64.shape
    assert close(loss, l64, LOSS_TOL)
    assert not bad.any()
    assert np.all(grad[g64 == 0] == 0)
    if w is None:   # the fraction is the designed count, exactly
        assert cnt64 == float(conf.sum()) and cm == np.float32(float(conf.sum()) / conf.numel())
    else:
        assert close(cm, cm64, LOSS_TOL)
    return loss, cm, grad, (l64, g64)


# ---- softmax consistency ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 2, 3, 19, 33, 64])
def test_consistency_softmax(hip_device, C):
    for hw in ((17, 31), (7, 9)):
        s, t, conf = design((2, C) + hw, seed=C)
        if C > 1:
            assert 0 < int(conf.sum()) < conf.numel()
        check_cons(f'C={C}', s, t, conf, hip_device, gout=0.75)


@pytest.mark.parametrize('C', [4, 5, 8, 9, 16, 17, 32])
def test_consistency_softmax_channel_bucket_edges(hip_device, C):
    s, t, conf = design((2, C, 17, 31), seed=40 + C)
    assert 0 < int(conf.sum()) < conf.numel()
    check_cons(f'bucket edge C={C}', s, t, conf, hip_device)


def test_consistency_softmax_second_round(hip_device):
    """exact_losses.S_GRID: past one round of the reduction (RED_SPAN) and of the element-wise grid (GRID_SPAN), more
    than 256 partials in the final block, more tiles than workgroups; every element of the gradient"""
    shape = tuple(E.S_GRID)
    assert shape == (3, 2, 1, 349_623)
    npix = shape[0] * shape[2] * shape[3]
    assert npix > E.GRID_SPAN > E.RED_SPAN
    s, t, conf = design(shape, seed=7)
    assert 0 < int(conf.sum()) < conf.numel()
    # gout scales the gradient back to O(1) per element so that the relative bound is the one that binds
    check_cons('S_GRID', s, t, conf, hip_device, gout=float(conf.sum()) / 16)


def test_consistency_softmax_weights(hip_device):
    s, t, conf = design((2, 19, 17, 31), seed=3)
    a = device_cons(s, t, THR, None, hip_device)
    b = device_cons(s, t, THR, torch.ones(2, 17, 31), hip_device)
    for x, y in zip(a, b):   # w == NULL gives the bits of w == 1
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    g = torch.Generator().manual_seed(11)
    w = torch.rand(2, 17, 31, generator=g)
    w[torch.rand(2, 17, 31, generator=g) < 0.25] = 0.0
    assert int((w == 0).sum()) > 50 and int(((w > 0) & conf).sum()) > 50
    _, _, grad, _ = check_cons('weighted', s, t, conf, hip_device, w=w)
    assert np.all(grad.transpose(0, 2, 3, 1)[(w == 0).numpy()] == 0)


def test_consistency_softmax_no_confident_pixel(hip_device):
    s, t, conf = design((2, 5, 7, 9), seed=5, frac=0.0)
    assert int(conf.sum()) == 0
    from ssseg import ops
    loss, cm = ops.consistency_loss_softmax(s.to(hip_device), t.to(hip_device), THR)
    print('no confident pixel:', float(loss), float(cm))
    assert torch.isnan(loss).item() and float(cm) == 0.0


def test_consistency_softmax_huge_logits(hip_device):
    for C in (3, 19):
        s, t, conf = design((2, C, 17, 31), seed=60 + C, scale=1e4)
        assert float(t.abs().max()) > 1e4 and 0 < int(conf.sum()) < conf.numel()
        loss, cm, grad, _ = check_cons(f'1e4 C={C}', s, t, conf, hip_device)
        assert np.isfinite(loss) and np.isfinite(grad).all() and loss > 0


def test_consistency_softmax_refuses_65_channels(hip_device):
    from ssseg import ops
    x = torch.zeros(2, 65, 7, 9, device=hip_device)
    with pytest.raises(ValueError, match='65 channels'):
        ops.consistency_loss_softmax(x, x, THR)
    with pytest.raises(ValueError, match='one shape'):
        ops.consistency_loss_softmax(x[:, :3], x[:, :4], THR)


def test_consistency_comparison_can_fail(hip_device):
    """a negated gradient, and the sigmoid loss in the softmax's place, both break the bounds at C = 3"""
    s, t, conf = design((2, 3, 17, 31), seed=9)
    loss, _, grad, (l64, g64) = check_cons('C=3', s, t, conf, hip_device)
    assert not close(-grad, g64, GRAD_TOL) and not close(0 * grad, g64, GRAD_TOL)
    ls, _, _, gs = R.consistency_softmax_grad(s, t, THR, activation='sigmoid')
    print(f'sigmoid reference: loss {ls!r} (softmax {l64!r}), grad max diff {_maxabs(gs - g64):.3e}')
    assert not close(loss, ls, LOSS_TOL) and not close(grad, gs, GRAD_TOL)


# ---- metrics ---------------------------------------------------------------------------------------------------------
def check_metrics(name, seg, logits, target, dev, total=None):
    want = R.seg_metrics(logits, target, seg.ignore, total)
    out = seg.update(logits.to(dev), target.to(dev)).cpu().double().numpy()
    C = seg.num_classes
    run = want['conf'] if total is None else total + want['conf']
    print(f'{name}: dice {out[0]!r} ({want["dice_mean"]!r}) mean IoU {out[1]!r} ({want["miou"]!r}) pixels counted '
          f'{int(seg.counts.sum())}')
    assert seg.counts.dtype == torch.int64 and torch.equal(seg.counts.cpu(), want['conf'])
    assert torch.equal(seg.dice.cpu(), want['dice'])
    assert torch.equal(seg.total.cpu(), run)
    assert out.shape == (2 + C,)
    assert np.allclose(out[0], want['dice_mean'], rtol=1e-6, atol=0)
    assert np.allclose(out[1], want['miou'], rtol=1e-6, atol=0)
    assert np.allclose(out[2:], 100 * want['ious'], rtol=1e-6, atol=0)
    return want, out


def _onehot_mask(label, C):
    return F.one_hot(label, C).permute(0, 3, 1, 2).float().contiguous()


@pytest.mark.parametrize('B,C,h,w,H,W', [(3, 19, 24, 24, 37, 37), (2, 64, 5, 7, 5, 7)])
def test_seg_metrics(hip_device, B, C, h, w, H, W):
    from ssseg import ops
    g = torch.Generator().manual_seed(C)
    logits = torch.randn(B, C, h, w, generator=g)
    mask = _onehot_mask(torch.randint(0, C, (B, H, W), generator=g), C)
    seg = ops.SegMetricsMC(hip_device, C)
    want, _ = check_metrics(f'C={C}', seg, logits, mask, hip_device)
    assert int(want['conf'].sum()) == B * H * W
    # a second update accumulates in the running total, and the IoUs come from it
    logits2 = torch.randn(B, C, h, w, generator=g)
    check_metrics(f'C={C} second batch', seg, logits2, mask, hip_device, total=want['conf'])


def test_seg_metrics_strided_views(hip_device):
    from ssseg import ops
    g = torch.Generator().manual_seed(1)
    B, C, h, w, H, W = 3, 19, 24, 24, 37, 37
    logits = torch.randn(B, h, w, C, generator=g).to(hip_device).permute(0, 3, 1, 2)        # channels-last view
    big = torch.zeros(B, C, 2 * H, W + 3)
    big[:, :, ::2, 3:] = _onehot_mask(torch.randint(0, C, (B, H, W), generator=g), C)
    mask = big.to(hip_device)[:, :, ::2, 3:]
    assert not logits.is_contiguous() and not mask.is_contiguous()
    check_metrics('strided', ops.SegMetricsMC(hip_device, C), logits, mask, hip_device)


def test_seg_metrics_ties_nan_and_absent_class(hip_device):
    from ssseg import ops
    g = torch.Generator().manual_seed(2)
    B, C, H, W = 2, 5, 13, 11
    # integer-valued logits and multi-hot masks: ties everywhere, the first index wins; class 3 never leads
    logits = torch.randint(0, 3, (B, C, H, W), generator=g).float()
    logits[:, 3] = -1.0
    mask = torch.randint(0, 2, (B, C, H, W), generator=g).float()
    mask[:, 3] = 0.0
    mask[:, 0] = torch.maximum(mask[:, 0], (mask.sum(1) == 0).float())      # an all-zero pixel would tie at class 0
    logits[0, 2, 4, 5] = float('nan')                                        # NaN is the maximum
    logits[1, 0, 0, 0] = float('nan')
    want, out = check_metrics('ties', ops.SegMetricsMC(hip_device, C), logits, mask, hip_device)
    assert int(want['conf'][3].sum()) == 0 and int(want['conf'][:, 3].sum()) == 0
    assert out[2 + 3] == 100.0                                               # absent from labels and predictions
    assert int(want['conf'][:, 2].sum()) > 0


def test_seg_metrics_label_map_with_ignore(hip_device):
    from ssseg import ops
    g = torch.Generator().manual_seed(3)
    B, C, h, w, H, W = 3, 19, 24, 24, 37, 37
    logits = torch.randn(B, C, h, w, generator=g)
    label = torch.randint(0, C, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.2] = 255
    frac = float((label == 255).float().mean())
    assert 0.15 < frac < 0.25
    seg = ops.SegMetricsMC(hip_device, C, ignore=255)
    want, _ = check_metrics('label map', seg, logits, label, hip_device)
    assert int(want['conf'].sum()) == int((label != 255).sum())
    # the dense one-hot mask of the same labels (no void pixels) counts what the label map counts
    label2 = torch.randint(0, C, (B, H, W), generator=g)
    a = ops.SegMetricsMC(hip_device, C)
    b = ops.SegMetricsMC(hip_device, C)
    oa = a.update(logits.to(hip_device), label2.to(hip_device))
    ob = b.update(logits.to(hip_device), _onehot_mask(label2, C).to(hip_device))
    assert torch.equal(a.counts, b.counts) and torch.equal(a.dice, b.dice) and torch.equal(oa, ob)


def test_seg_metrics_two_classes_equal_the_binary_kernel(hip_device):
    from ssseg import ops
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(3, 2, 24, 24, generator=g).to(hip_device)
    mask = _onehot_mask(torch.randint(0, 2, (3, 37, 37), generator=g), 2).to(hip_device)
    old, new = ops.SegMetrics(hip_device), ops.SegMetricsMC(hip_device, 2)
    for _ in range(2):
        o, n = old.update(logits, mask).cpu(), new.update(logits, mask).cpu()
        print('binary', o.tolist(), 'C-class', n.tolist())
        assert o[0] == n[0] and o[1] == n[2] and o[2] == n[3]
        assert abs(float(o[3]) - 100 * float(n[1])) <= 1e-6 * float(o[3])
        logits = logits.flip(0)


# ---- inference head --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ['sigmoid', 'softmax'])
@pytest.mark.parametrize('C', [2, 5, 64])
def test_prob_onehot(hip_device, C, activation):
    from ssseg import ops
    g = torch.Generator().manual_seed(C)
    x = 3 * torch.randn(2, C, 17, 31, generator=g)
    x[0, 0, 0, :5] = x[0, C - 1, 0, :5] = 9.0          # ties: the first index wins
    x[1, C // 2, 3, 4] = 50.0
    prob, onehot = ops.prob_onehot(x.to(hip_device), activation)
    p64, oh = R.prob_onehot(x, activation)
    err = (prob.cpu().double() - p64).abs().max()
    print(f'C={C} {activation}: max |p - fp64| {float(err):.3e}')
    assert prob.shape == x.shape and prob.dtype == torch.float32
    assert torch.equal(onehot.cpu(), oh)
    assert close(prob.cpu().numpy(), p64.numpy(), LOSS_TOL)
    if activation == 'softmax':
        assert close(prob.sum(1).cpu().numpy(), 1.0, LOSS_TOL)


def test_prob_onehot_nan_is_the_maximum(hip_device):
    from ssseg import ops
    x = torch.randn(1, 5, 3, 3)
    x[0, 3, 1, 1] = float('nan')
    _, onehot = ops.prob_onehot(x.to(hip_device), 'sigmoid')
    assert torch.equal(onehot.cpu(), R.prob_onehot(x)[1]) and onehot[0, 3, 1, 1] == 1


def _small_pair(C, dev, head_gain=6.0):
    """SimpleUNet(C, 2 blocks, 8 channels) student / teacher on the device and their oracle twins, the logit head
    scaled and the BatchNorm statistics warmed up so that the teacher's softmax confidence straddles 0.5 (an untrained
    head with fresh statistics is nowhere confident at C = 5)"""
    from models import simple_unet
    from models.adapters import ListOutput
    from oracle import models_ref
    torch.manual_seed(0)
    ref_s = models_ref.ListOutput(models_ref.SimpleUNet(C, 2, 8, 16))
    ref_t = models_ref.ListOutput(models_ref.SimpleUNet(C, 2, 8, 16))
    with torch.no_grad():
        ref_s.model.final_block[1].weight.mul_(head_gain)
        # BatchNorm running statistics of the data (fresh ones leave the eval-mode teacher's logits near zero)
        g = torch.Generator().manual_seed(123)
        ref_s.train()
        for _ in range(40):
            ref_s(torch.rand(2, 3, 64, 64, generator=g))
    ref_t.load_state_dict(ref_s.state_dict())
    student = ListOutput(simple_unet.UNet(C, 2, 8, 16))
    teacher = ListOutput(simple_unet.UNet(C, 2, 8, 16))
    student.load_state_dict(ref_s.state_dict())
    teacher.load_state_dict(ref_s.state_dict())
    student, teacher = student.to(dev), teacher.to(dev)
    for m in (teacher, ref_t):
        for p in m.parameters():
            p.detach_()
        m.eval()
    return student, teacher, ref_s, ref_t


class _Spy(torch.nn.Module):
    """records the last logit map of every forward"""

    def __init__(self, m):
        super().__init__()
        self.m, self.seen = m, []

    def forward(self, x):
        f, p = self.m(x)
        self.seen.append(p[-1].detach().float())
        return f, p


@pytest.fixture
def fp32_compute():
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.float32)
    yield
    snn.set_compute_dtype(torch.bfloat16)


def test_inference_wrapper(hip_device, fp32_compute):
    from models.inference_wrapper import InferenceWrapper
    from ssseg import native as N
    from ssseg import ops
    image = torch.rand(3, 40, 56, generator=torch.Generator().manual_seed(1)).to(hip_device)
    with torch.no_grad():
        model2 = _Spy(_small_pair(2, hip_device)[0].eval())
        mask, prob = InferenceWrapper(model2)(image)
        # the wrapper's output path as it was: bilinear resize + ssseg_prob_onehot on the same logits
        x = ops.interpolate_bilinear(model2.seen[-1], [40, 56], align_corners=False).contiguous()
        p0, m0 = torch.empty_like(x), torch.empty_like(x)
        N.call('ssseg_prob_onehot', N.dev_ptr(x), 1, 40 * 56, N.dev_ptr(p0), N.dev_ptr(m0), N.stream())
        assert torch.equal(mask, m0[0]) and torch.equal(prob, p0[0]) and mask.shape == (2, 40, 56)
        model5 = _Spy(_small_pair(5, hip_device)[0].eval())
        for act in ('sigmoid', 'softmax'):
            mask, prob = InferenceWrapper(model5, activation=act)(image)
            x5 = ops.interpolate_bilinear(model5.seen[-1], [40, 56], align_corners=False)
            p64, oh = R.prob_onehot(x5, act)
            assert mask.shape == (5, 40, 56) and torch.equal(mask.cpu(), oh[0])
            assert close(prob.cpu().numpy(), p64[0].numpy(), LOSS_TOL)


# ---- the training step -----------------------------------------------------------------------------------------------
def _tcfg(activation=None, **over):
    import losses
    tc = dict(loss=losses.CalculateLoss([{'loss_fn': losses.DenseBinaryCrossEntropyLossWithLogits('mean'),
                                          'weight': [0.5]}]),
              virtual_batch_size_multiplier=1, use_semi_supervised=True, mask_proportion_range=(0.45, 0.55),
              sigma_range=(2, 4), confidence_threshold=0.5, consistency_loss_weight=10, ema_model_alpha=0.99,
              print_freq=1, gradient_clip_value=5.0)
    if activation is not None:
        tc['consistency_activation'] = activation
    tc.update(over)
    return tc


def _step_data(C, steps, size=64, batch=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand(steps, batch, 3, size, size, generator=g)
    masks = _onehot_mask(torch.randint(0, C, (steps * batch, size, size), generator=g), C)
    unl = torch.rand(2 * steps, batch, 3, size, size, generator=g)
    return imgs, masks.view(steps, batch, C, size, size), unl


def test_softmax_step_vs_oracle(hip_device, fp32_compute, monkeypatch):
    """three semi-supervised steps of a 5-class SimpleUNet at 64^2, batch 2, epoch 26, threshold 0.5, against the
    oracle's train_epoch with its consistency_loss swapped for the softmax restatement"""
    import copy

    import cowmix
    import train
    from oracle import train_ref
    from parity import check_losses, tensor_outliers
    from ssseg import arena, optim
    monkeypatch.setattr(train_ref, 'consistency_loss', lambda s, t, thr: R.consistency_softmax(s, t, thr)[:2])
    C, steps = 5, 3
    student, teacher, ref_s, ref_t = _small_pair(C, hip_device)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps)
    tc = _tcfg('softmax')

    def oracle(dt, pert=0.0):
        s, t = copy.deepcopy(ref_s).to(dt), copy.deepcopy(ref_t).to(dt)
        o = torch.optim.SGD(s.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        x, u = imgs.to(dt), unl.to(dt)
        if pert:   # the step's own sensitivity (tests/parity.py): inputs moved by ~fp32 rounding
            gp = torch.Generator().manual_seed(99)
            x = x * (1 + pert * torch.randn(x.shape, generator=gp, dtype=dt))
            u = u * (1 + pert * torch.randn(u.shape, generator=gp, dtype=dt))
        g0 = {}

        def grab(step, rec):   # step 0 runs no optimizer step (train.py:121): its gradients are still in .grad
            if step == 0:
                g0.update({k: p.grad.detach().double().numpy().copy() for k, p in s.named_parameters()})
        torch.manual_seed(3)
        logs = train_ref.train_epoch(s, t, o, list(zip(x, masks.to(dt))), iter(u), 26,
                                     train_ref.default_cfg(sigma_range=(2, 4), confidence_threshold=0.5),
                                     on_step=grab)
        return logs, s, g0
    r32, s32, g32 = oracle(torch.float32)
    r64, s64, g64 = oracle(torch.float64)
    _, sp, gp = oracle(torch.float64, pert=1e-6)
    print('oracle fp64:', r64)
    assert all(0.02 < r['cm_mean'] < 0.98 and r['unsup_loss'] > 0 for r in r64)    # the gate is open, both kinds of pixel
    old = cowmix.NOISE_SOURCE
    cowmix.NOISE_SOURCE = 'cpu'
    try:
        torch.manual_seed(3)
        student.train()
        opt.zero_grad()
        logs = []
        for k in range(steps):
            c, u, cm = train.train_step(student, teacher, opt, imgs[k].to(hip_device), masks[k].to(hip_device),
                                        unl[2 * k].to(hip_device), unl[2 * k + 1].to(hip_device), 26, k, {'train': tc})
            logs.append((float(c), float(u)))
            print(f'step {k}: sup {float(c)!r} unsup {float(u)!r} cm {float(cm)!r}')
            if k == 0:
                ghip = {n: p.grad.detach().cpu().double().numpy().copy() for n, p in student.named_parameters()}
    finally:
        cowmix.NOISE_SOURCE = old
    check_losses(logs, [(r['sup_loss'], r['unsup_loss']) for r in r32],
                 [(r['sup_loss'], r['unsup_loss']) for r in r64])
    gfloor = 1e-3 * max(float(np.abs(v).max()) for v in g64.values())
    gbad = tensor_outliers(ghip, g32, g64, gp, floor=gfloor)
    print('step-0 gradient outliers:', gbad[:5])
    assert not gbad, gbad[:5]
    np_sd = lambda m: {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items()}  # noqa: E731
    sd64 = np_sd(s64)
    floor = 1e-3 * max(float(np.abs(v).max()) for k, v in sd64.items() if 'running' not in k and v.ndim)
    bad = tensor_outliers(np_sd(student), np_sd(s32), sd64, np_sd(sp), floor=floor, factor=4.0)
    print('parameter outliers after 3 steps:', bad[:5])
    assert not bad, bad[:5]


def _device_steps(C, dev, tc, graphed=False, steps=3):
    """2 eager steps + `steps` more (eager, or replays of one captured step), CowMix drawn on the device"""
    import cowmix
    import train
    from ssseg import arena, optim
    from ssseg.graph import StepGraph
    student, teacher, _, _ = _small_pair(C, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps + 2)
    data = [(imgs[k].to(dev), masks[k].to(dev), unl[2 * k].to(dev), unl[2 * k + 1].to(dev)) for k in range(steps + 2)]
    cfg = {'train': tc}
    assert cowmix.NOISE_SOURCE == 'device'
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    student.train()
    opt.zero_grad()
    out = [train.train_step(student, teacher, opt, *data[k], 26, k, cfg) for k in range(2)]
    if graphed:
        g = StepGraph(lambda i, m, a, b: train.train_step(student, teacher, opt, i, m, a, b, 26, 2, cfg), *data[2])
        for k in range(2, steps + 2):
            out.append(tuple(t.clone() for t in g(*data[k])))
    else:
        for k in range(2, steps + 2):
            out.append(train.train_step(student, teacher, opt, *data[k], 26, k, cfg))
    torch.cuda.synchronize()
    state = {**{'s.' + k: v.detach().clone() for k, v in student.state_dict().items()},
             **{'t.' + k: v.detach().clone() for k, v in teacher.state_dict().items()}}
    # the key of the next step's captured graph under either activation (one config object, the value changed)
    cfg2 = {'train': dict(tc)}
    keys = []
    for act in ('sigmoid', 'softmax'):
        cfg2['train']['consistency_activation'] = act
        keys.append(train._graph_key(student, teacher, opt, *data[0], 26, steps + 2, cfg2))
    state['graph_keys'] = keys
    return [tuple(float(t) for t in l) for l in out], state


def test_softmax_step_graph_replay_matches_eager_bitwise(hip_device, fp32_compute):
    eager, s_e = _device_steps(5, hip_device, _tcfg('softmax'))
    graph, s_g = _device_steps(5, hip_device, _tcfg('softmax'), graphed=True)
    print('eager', eager, 'graph', graph)
    assert np.array_equal(np.array(eager), np.array(graph), equal_nan=True)
    assert all(np.isfinite(l).all() and l[1] > 0 and 0 < l[2] < 1 for l in eager)
    keys = s_e.pop('graph_keys')
    s_g.pop('graph_keys')
    assert keys[0] is not None and keys[1] is not None and keys[0] != keys[1]   # a replay repeats its capture's choice
    for k in s_e:
        assert torch.equal(s_e[k], s_g[k]), k


def test_activation_key_default_and_two_class_difference(hip_device, fp32_compute):
    """a config without the key gives the bits of 'sigmoid'; at C = 2 'softmax' is another unsupervised loss"""
    import train
    none, s_n = _device_steps(2, hip_device, _tcfg(None), steps=1)
    sig, s_s = _device_steps(2, hip_device, _tcfg('sigmoid'), steps=1)
    soft, _ = _device_steps(2, hip_device, _tcfg('softmax'), steps=1)
    print('no key', none, 'sigmoid', sig, 'softmax', soft)
    s_n.pop('graph_keys'), s_s.pop('graph_keys')
    assert none == sig and all(torch.equal(s_n[k], s_s[k]) for k in s_n)
    assert all(a[0] == b[0] for a, b in zip(sig[:1], soft[:1]))        # the supervised loss of step 0 is the same
    assert all(np.isfinite(a[1]) and np.isfinite(b[1]) and a[1] != b[1] for a, b in zip(sig, soft))
    with pytest.raises(ValueError, match='consistency_activation'):
        train._consistency_activation({'consistency_activation': 'tanh'})


def test_validate_multiclass(hip_device, fp32_compute):
    """train.validate on a 5-class synthetic loader: returns, and its mIoU is the CPU restatement's"""
    import train
    from data.synthetic import SyntheticSegDataset
    C = 5
    student = _small_pair(C, hip_device)[0]
    spy = _Spy(student)
    ds = SyntheticSegDataset(length=6, size=64, seed=4, blob_sigma=4.0, num_classes=C)
    loader = torch.utils.data.DataLoader(ds, batch_size=2)
    loss, metric = train.validate(spy, loader, 0, 0, None, {'train': _tcfg()}, hip_device)
    total, dices = None, []
    seen = [t.cpu() for t in spy.seen]
    for logits, sample in zip(seen, loader):
        m = R.seg_metrics(logits, sample['semantic_mask'], total=total)
        total = m['conf'] if total is None else total + m['conf']
        dices.append(m['dice_mean'])
    print(f'validate: loss {float(loss)!r} dice {float(metric)!r} ({np.mean(dices)!r}) mIoU {train._VALIDATE["miou"]!r} '
          f'({100 * m["miou"]!r})')
    assert len(seen) == 3 and np.isfinite(float(loss))
    assert np.allclose(float(metric), np.mean(dices), rtol=1e-6, atol=0)
    assert np.allclose(train._VALIDATE['miou'], 100 * m['miou'], rtol=1e-6, atol=0)
    assert np.allclose(train._VALIDATE['class_ious'], 100 * m['ious'], rtol=1e-6, atol=0)
