"""GPU: the pseudo-label consistency loss (ssseg_consistency_ce_fwd / _bwd in csrc/multiclass.hip) through
ops.consistency_loss_ce and the training step that selects it with train['consistency_loss'] = 'ce', against the fp64
restatement of tests/pseudo_ce_ref.py.

Bounds: the project's loss bounds, imported from test_hip_losses_ext.py: loss rtol 2e-5 atol
1e-7; gradient rtol 2e-4 atol 2e-8 at every element, exactly 0.0 wherever the fp64 gradient is 0; the step against the
oracle under the rules of tests/parity.py.  Teacher logits are multiclass_ref.confident_teacher's: every pixel's
max softmax is at least 1e-3 from the threshold (asserted), and its unconfident pixels carry a designed exact tie of two
channels, which the first-maximum rule has to place.  The kernel's own thresholds: the 256-pixel tile (17*31 = 527
pixels per sample), the channel buckets 2, 4, 8, 16, 32, 64 of the backward and the 8-channel chunks of both passes
(C = 8, 9, 16, 17 sit on both sides of a chunk edge), more tiles than workgroups (S_GRID).  Every test prints its
figures before it asserts.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_losses as E
import multiclass_ref as R
import pseudo_ce_ref as P
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL
from test_multiclass import THR, _maxabs, _small_pair, _step_data, _tcfg, close, design, fp32_compute  # noqa: F401

pytestmark = pytest.mark.gpu

WEIGHTINGS = ('pixel', 'batch')


def device_ce(s, t, thr, w, weighting, dev, gout=1.0):
    """-> (loss, cm mean, gradient of gout * loss) as numpy"""
    from ssseg import ops
    x = s.to(dev).requires_grad_(True)
    loss, cm = ops.consistency_loss_ce(x, t.to(dev), thr, None if w is None else w.to(dev), weighting)
    assert not cm.requires_grad
    (loss * gout).backward()
    return loss.detach().cpu().numpy(), cm.detach().cpu().numpy(), x.grad.cpu().numpy()


def weight_maps(shape, seed):
    """the w operands of one shape: none, ones, a 0-1 map, a fractional map with zeros"""
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed + 500)
    binary = (torch.rand(B, H, W, generator=g) > 0.3).float()
    frac = torch.rand(B, H, W, generator=g)
    frac[torch.rand(B, H, W, generator=g) < 0.25] = 0.0
    return {'none': None, 'ones': torch.ones(B, H, W), 'binary': binary, 'fractional': frac}


def check_ce(name, s, t, conf, dev, w, weighting, gout, ref=P.pseudo_ce_grad):
    l64, cm64, scm64, g64 = ref(s, t, THR, w, weighting, gout)
    loss, cm, grad = device_ce(s, t, THR, w, weighting, dev, gout)
    bad = ~np.isclose(grad, g64, equal_nan=True, **GRAD_TOL)
    print(f'{name} {tuple(s.shape)} {weighting}: loss dev {loss!r} fp64 {l64!r} rel {abs(loss - l64) / abs(l64 + 1e-300):.2e}'
          f' | cm {cm!r} fp64 {cm64!r} | grad dev-fp64 {_maxabs(grad - g64):.3e} of {_maxabs(g64):.3e}, '
          f'{int(bad.sum())} of {bad.size} out of bound')
    assert loss.dtype == np.float32 and grad.shape == g64.shape
    assert close(loss, l64, LOSS_TOL)
    assert not bad.any()
    assert np.all(grad[g64 == 0] == 0)
    if w is None:   # the fraction is the designed count, exactly
        assert scm64 == float(conf.sum()) and cm == np.float32(float(conf.sum()) / conf.numel())
    else:
        assert close(cm, cm64, LOSS_TOL)
    return loss, cm, grad, (l64, g64)


def check_shape(shape, seed, dev, maps=('none', 'ones', 'binary', 'fractional')):
    s, t, conf = design(shape, seed=seed)
    if shape[1] > 1:
        assert 0 < int(conf.sum()) < conf.numel()
    ws = weight_maps(shape, seed)
    # gout scales the gradient to O(1 / 16) per pixel so that the relative bound is the one that binds
    gout = conf.numel() / 16.0
    for weighting in WEIGHTINGS:
        got = {k: check_ce(f'w={k}', s, t, conf, dev, ws[k], weighting, gout) for k in maps}
        if 'ones' in got:   # w == NULL gives the bits of w == 1
            for a, b in zip(got['none'][:3], got['ones'][:3]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for k in ('binary', 'fractional'):
            if k in got:
                assert int((ws[k] == 0).sum()) > 10 and int(((ws[k] > 0) & conf).sum()) > 10
                assert np.all(got[k][2].transpose(0, 2, 3, 1)[(ws[k] == 0).numpy()] == 0)
        if weighting == 'pixel':
            assert np.all(got['none'][2].transpose(0, 2, 3, 1)[(~conf).numpy()] == 0)


# ---- 1. loss and gradient against fp64 -------------------------------------------------------------------------------
def test_less_than_a_wave(hip_device):
    check_shape((2, 3, 7, 9), 3, hip_device)


@pytest.mark.parametrize('C', [1, 2, 3, 4, 5, 8, 9, 16, 17, 19, 32, 33, 64])
def test_channel_buckets_and_tiles(hip_device, C):
    check_shape((2, C, 17, 31), 40 + C, hip_device)


def test_more_tiles_than_workgroups(hip_device):
    """exact_losses.S_GRID: 4098 tiles on 1024 (forward) / 4096 (backward) workgroups, more than 256 partials in the
    final block; every element of the gradient"""
    shape = tuple(E.S_GRID)
    assert shape == (3, 2, 1, 349_623) and shape[0] * ((shape[3] + 255) // 256) == 4098
    check_shape(shape, 7, hip_device, maps=('none', 'fractional'))


# ---- 2. the comparison can fail --------------------------------------------------------------------------------------
def test_comparison_can_fail(hip_device):
    """a negated gradient, the MSE loss in the CE's place and 'batch' in the place of 'pixel' all break the bounds"""
    s, t, conf = design((2, 3, 17, 31), seed=9)
    gout = conf.numel() / 16.0
    loss, _, grad, (l64, g64) = check_ce('C=3', s, t, conf, hip_device, None, 'pixel', gout)
    assert not close(-grad, g64, GRAD_TOL) and not close(0 * grad, g64, GRAD_TOL)
    lm, _, _, gm = R.consistency_softmax_grad(s, t, THR, None, gout)
    print(f'MSE reference: loss {lm!r} (CE {l64!r}), grad max diff {_maxabs(gm - g64):.3e}')
    assert not close(loss, lm, LOSS_TOL) and not close(grad, gm, GRAD_TOL)
    lb, _, _, gb = P.pseudo_ce_grad(s, t, THR, None, 'batch', gout)
    print(f"'batch' reference: loss {lb!r}, grad max diff {_maxabs(gb - g64):.3e}")
    assert not close(loss, lb, LOSS_TOL) and not close(grad, gb, GRAD_TOL)
    with pytest.raises(AssertionError):
        check_ce('batch for pixel', s, t, conf, hip_device, None, 'pixel', gout,
                 ref=lambda s, t, thr, w, weighting, gout: P.pseudo_ce_grad(s, t, thr, w, 'batch', gout))


# ---- 3. the argmax rule ----------------------------------------------------------------------------------------------
def test_argmax_rule_ties_and_nan(hip_device):
    """the label is torch.argmax's: shown by where the gradient is negative (softmax(s)_c - [c == y] < 0 only at y),
    under 'batch', where every pixel has a gradient; and the forward's own pick of s[y] by the loss"""
    nan = float('nan')
    rows = [[1.0, 3.0, 0.0, 3.0, 2.0],        # two-way tie: the first maximum, 1
            [2.0, 0.0, 2.0, -1.0, 2.0],       # three-way tie: 0
            [0.0, 4.0, 4.0, 4.0, 1.0],        # three-way tie inside: 1
            [0.0, 0.0, 0.0, 0.0, 0.0],        # all equal: 0
            [1.0, 2.0, nan, 9.0, 3.0],        # NaN counts as the maximum, also before a larger value: 2
            [1.0, nan, 5.0, nan, 0.0],        # the first NaN: 1
            [nan, 7.0, 1.0, 2.0, 3.0],        # NaN in channel 0: 0
            [-1.0, -2.0, -3.0, -0.5, -0.5]]   # a tie in the last two: 3
    want = torch.tensor([1, 0, 1, 0, 2, 1, 0, 3])
    for C in (5, 9):    # one chunk, and the same rows spread over two 8-channel chunks (channel c -> 2c)
        t = torch.full((2, C, 2, 4), -50.0)
        src = torch.tensor(rows).t().reshape(5, 2, 4)
        step = 1 if C == 5 else 2
        t[0, ::step] = src
        t[1, ::step] = src.flip(2)
        label = torch.stack([want.view(2, 4), want.view(2, 4).flip(1)]) * step
        assert torch.equal(torch.argmax(t, 1), label)
        s = torch.randn(2, C, 2, 4, generator=torch.Generator().manual_seed(C))
        onehot = F.one_hot(label, C).permute(0, 3, 1, 2).bool()
        # (every finite row's max softmax is at least 0.013 from 0.3; the all-equal row and the NaN rows are below)
        loss, cm, grad = device_ce(s, t, 0.3, None, 'batch', hip_device, gout=16.0)
        l64, cm64, _, g64 = P.pseudo_ce_grad(s, t, 0.3, None, 'batch', gout=16.0)
        print(f'C={C}: loss {loss!r} fp64 {l64!r} cm {cm!r} fp64 {cm64!r}')
        assert torch.equal(torch.from_numpy(grad < 0), onehot)
        assert np.isfinite(grad).all() and close(loss, l64, LOSS_TOL) and close(grad, g64, GRAD_TOL)
        assert cm == np.float32(cm64) and 0 < cm < 1
        # under 'pixel' a NaN teacher pixel is not confident: exact zeros there, the label's sign pattern elsewhere
        _, _, grad = device_ce(s, t, 0.3, None, 'pixel', hip_device, gout=16.0)
        on = torch.softmax(t.double(), 1).amax(1) > 0.3
        assert 0 < int(on.sum()) < on.numel()
        assert torch.equal(torch.from_numpy(grad < 0), onehot & on.unsqueeze(1))
        assert np.all(grad.transpose(0, 2, 3, 1)[(~on).numpy()] == 0)


# ---- 4. selected, not multiplied -------------------------------------------------------------------------------------
def test_unconfident_pixels_are_selected_out(hip_device):
    from ssseg import ops
    for C in (3, 19):
        s, t, conf = design((2, C, 17, 31), seed=70 + C)
        assert 0 < int(conf.sum()) < conf.numel()
        g = torch.Generator().manual_seed(C)
        wild = torch.tensor([1e4, -1e4, float('nan')])[torch.randint(0, 3, s.shape, generator=g)]
        s_wild = torch.where(conf.unsqueeze(1), s, wild)
        assert int(torch.isnan(s_wild).sum()) > 50 and torch.isfinite(s_wild[conf.unsqueeze(1).expand_as(s)]).all()
        gout = conf.numel() / 16.0
        loss, cm, grad = device_ce(s_wild, t, THR, None, 'pixel', hip_device, gout)
        l64 = P.pseudo_ce(s_wild.double(), t.double(), THR)[0].numpy()           # the forward on the wild student itself
        # (autograd through torch.where gives 0 * NaN at the selected-out pixels: the gradient's yardstick is the fp64
        # gradient on the student with those pixels zeroed, which is the same loss)
        l64b, _, _, g64 = P.pseudo_ce_grad(torch.where(conf.unsqueeze(1), s, torch.zeros(())), t, THR, None, 'pixel', gout)
        print(f'C={C}: wild student loss dev {loss!r} fp64 {l64!r} (tame {l64b!r}); grad dev-fp64 {_maxabs(grad - g64):.3e}')
        assert l64 == l64b and np.isfinite(loss) and close(loss, l64, LOSS_TOL)
        assert close(grad, g64, GRAD_TOL)
        assert np.all(grad.transpose(0, 2, 3, 1)[(~conf).numpy()] == 0)
        # 'batch' multiplies: the same student poisons it, like the restatement
        lb, _, _ = device_ce(s_wild, t, THR, None, 'batch', hip_device)
        assert np.isnan(lb) and np.isnan(P.pseudo_ce(s_wild.double(), t.double(), THR, None, 'batch')[0].numpy())
        # no confident pixel at all: exactly 0.0 and an all-zero gradient, where the squared-difference form is 0/0
        for student in (s, s_wild):
            loss, cm, grad = device_ce(student, t, 1.0, None, 'pixel', hip_device, gout)
            print(f'C={C} thr=1: loss {loss!r} cm {cm!r} grad max {np.abs(grad).max()!r}')
            assert loss == 0.0 and not np.signbit(loss) and cm == 0.0 and np.all(grad == 0)
        mse, mse_cm = ops.consistency_loss_softmax(s.to(hip_device), t.to(hip_device), 1.0)
        assert torch.isnan(mse).item() and float(mse_cm) == 0.0


def test_zero_weight_everywhere_is_nan(hip_device):
    s, t, _ = design((2, 5, 7, 9), seed=5)
    for weighting in WEIGHTINGS:
        loss, cm, _ = device_ce(s, t, THR, torch.zeros(2, 7, 9), weighting, hip_device)
        assert np.isnan(loss) and cm == 0.0


# ---- 5. host-side refusals -------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(hip_device):
    from ssseg import native as N
    from ssseg import ops
    x = torch.zeros(2, 65, 7, 9, device=hip_device)
    with pytest.raises(ValueError, match='65 channels'):
        ops.consistency_loss_ce(x, x, THR)
    with pytest.raises(ValueError, match='one shape'):
        ops.consistency_loss_ce(x[:, :3], x[:, :4], THR)
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.consistency_loss_ce(x[:, :3].cpu(), x[:, :3], THR)
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.consistency_loss_ce(x[:, :3], x[:, :3], THR, w=torch.ones(2, 7, 9))
    with pytest.raises(ValueError, match='weighting'):
        ops.consistency_loss_ce(x[:, :3], x[:, :3], THR, weighting='image')
    with pytest.raises(ValueError, match='one weight per pixel'):
        ops.consistency_loss_ce(x[:, :3], x[:, :3], THR, w=torch.ones(2, 7, 8, device=hip_device))
    # the entry points themselves: 65 channels and a weighting of 2 are SSSEG_EINVAL with device pointers too
    out, ws = torch.zeros(4, device=hip_device), torch.zeros(1 << 15, dtype=torch.uint8, device=hip_device)
    lib, p = N.lib(), N.dev_ptr
    assert lib.ssseg_consistency_ce_fwd(p(x), p(x), None, 2, 65, 63, THR, 0, p(out), p(ws), ws.numel(), None) == -1
    assert lib.ssseg_consistency_ce_fwd(p(x), p(x), None, 2, 3, 63, THR, 2, p(out), p(ws), ws.numel(), None) == -1
    assert lib.ssseg_consistency_ce_bwd(p(x), p(x), None, 2, 3, 63, THR, 2, p(out), p(out), p(x), None) == -1
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


# ---- 6. the training step --------------------------------------------------------------------------------------------
def _step_vs_oracle(dev, monkeypatch, weighting, aug):
    """three semi-supervised steps of a 5-class SimpleUNet at 64^2, batch 2, epoch 26, threshold 0.5, against the
    oracle's train_epoch with its consistency_loss swapped for the restatement (test_softmax_step_vs_oracle's frame)"""
    import copy

    import cowmix
    import train
    from oracle import train_ref
    from parity import check_losses, tensor_outliers
    from ssseg import arena, optim
    monkeypatch.setattr(train_ref, 'consistency_loss', lambda s, t, thr: P.pseudo_ce(s, t, thr, None, weighting)[:2])
    C, steps = 5, 3
    student, teacher, ref_s, ref_t = _small_pair(C, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps)
    tc = _tcfg('softmax', consistency_loss='ce', consistency_ce_weighting=weighting)
    if aug is not None:
        tc['consistency_augmentation'] = aug

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
    assert all(0.02 < r['cm_mean'] < 0.98 and r['unsup_loss'] > 0 for r in r64)    # both kinds of pixel occur
    old = cowmix.NOISE_SOURCE
    cowmix.NOISE_SOURCE = 'cpu'
    try:
        torch.manual_seed(3)
        student.train()
        opt.zero_grad()
        logs = []
        for k in range(steps):
            c, u, cm = train.train_step(student, teacher, opt, imgs[k].to(dev), masks[k].to(dev),
                                        unl[2 * k].to(dev), unl[2 * k + 1].to(dev), 26, k, {'train': tc})
            logs.append((float(c), float(u)))
            print(f'step {k}: sup {float(c)!r} unsup {float(u)!r} cm {float(cm)!r} (oracle fp64 {r64[k]["cm_mean"]!r})')
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


def test_step_vs_oracle_cowmix_pixel(hip_device, fp32_compute, monkeypatch):
    _step_vs_oracle(hip_device, monkeypatch, 'pixel', None)


def test_step_vs_oracle_batch_with_augmentation(hip_device, fp32_compute, monkeypatch):
    """'batch' through the consistency_augmentation path of the step (the view, the warp back, aug.valid as w).  The
    oracle's step has no warp, so the view is the identity (fixed parameters: angle 0, scale 1), whose warp returns its
    input bit for bit and whose validity map is all ones (test_geo_consistency.py)."""
    import reversible_augmentations as RA
    aug = RA.RotateRescale(15, 0.75, 1.25)
    aug.set_params([0.0, 0.0], [1.0, 1.0])
    _step_vs_oracle(hip_device, monkeypatch, 'batch', aug)
    assert aug.valid is not None and torch.equal(aug.valid, torch.ones_like(aug.valid))


# ---- 7. the captured step --------------------------------------------------------------------------------------------
def _device_steps(dev, tc, n_eager, n_graph=0):
    """n_eager eager steps, then n_graph replays of one captured step; CowMix drawn on the device.  -> (losses, the
    Philox counter after the last step, the graph keys of the next step under each loss choice)"""
    import cowmix
    import train
    from ssseg import arena, optim
    from ssseg.graph import StepGraph
    C = 5
    student, teacher, _, _ = _small_pair(C, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    n = n_eager + n_graph
    imgs, masks, unl = _step_data(C, n)
    data = [(imgs[k].to(dev), masks[k].to(dev), unl[2 * k].to(dev), unl[2 * k + 1].to(dev)) for k in range(n)]
    cfg = {'train': tc}
    assert cowmix.NOISE_SOURCE == 'device'
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    student.train()
    opt.zero_grad()
    out = [train.train_step(student, teacher, opt, *data[k], 26, k, cfg) for k in range(n_eager)]
    if n_graph:
        g = StepGraph(lambda i, m, a, b: train.train_step(student, teacher, opt, i, m, a, b, 26, n_eager, cfg),
                      *data[n_eager])
        for k in range(n_eager, n):
            out.append(tuple(t.clone() for t in g(*data[k])))
    torch.cuda.synchronize()
    ctr = int(cowmix._DEVICE_RNG['ctr'][dev.index if dev.index is not None else torch.cuda.current_device()])
    cfg2 = {'train': {k: v for k, v in tc.items() if k not in ('consistency_loss', 'consistency_ce_weighting')}}
    keys = {}
    for name, over in (('none', {}), ('mse', {'consistency_loss': 'mse'}), ('pixel', {'consistency_loss': 'ce'}),
                       ('batch', {'consistency_loss': 'ce', 'consistency_ce_weighting': 'batch'})):
        for k in ('consistency_loss', 'consistency_ce_weighting'):
            cfg2['train'].pop(k, None)
        cfg2['train'].update(over)      # one config object, the values changed
        keys[name] = train._graph_key(student, teacher, opt, *data[0], 26, n, cfg2)
    return [tuple(float(t) for t in l) for l in out], ctr, keys


@pytest.mark.parametrize('weighting', WEIGHTINGS)
def test_ce_step_graph_replay_matches_eager_bitwise(hip_device, fp32_compute, weighting):
    tc = lambda: _tcfg('softmax', consistency_loss='ce', consistency_ce_weighting=weighting)  # noqa: E731
    eager, ctr_e, keys = _device_steps(hip_device, tc(), 5)
    graph, ctr_g, _ = _device_steps(hip_device, tc(), 2, 3)
    print('eager', eager, 'graph', graph)
    assert np.array_equal(np.array(eager), np.array(graph), equal_nan=True) and ctr_e == ctr_g
    assert all(np.isfinite(l).all() and l[1] > 0 and 0 < l[2] < 1 for l in eager)
    # a replay repeats its capture's choice: every choice has a key of its own; no key is 'mse'
    assert all(k is not None for k in keys.values())
    assert keys['none'] == keys['mse'] and len({keys['mse'], keys['pixel'], keys['batch']}) == 3


def test_without_the_keys_is_mse_bitwise(hip_device, fp32_compute):
    none, ctr_n, _ = _device_steps(hip_device, _tcfg('softmax'), 2)
    mse, ctr_m, _ = _device_steps(hip_device, _tcfg('softmax', consistency_loss='mse'), 2)
    ce, ctr_c, _ = _device_steps(hip_device, _tcfg('softmax', consistency_loss='ce'), 2)
    print('no key', none, 'mse', mse, 'ce', ce)
    assert np.array(none).tobytes() == np.array(mse).tobytes() and ctr_n == ctr_m and ctr_n > 0
    assert ce[0][0] == mse[0][0] and ce[0][1] != mse[0][1] and ctr_c == ctr_m   # another loss on the same draws
