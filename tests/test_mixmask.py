"""ClassMix and CutMix masks on the device (csrc/mixmask.hip, ssseg.ops, mixmasks.py, train.py's mix_mask key) against
the CPU restatements of tests/mixmask_ref.py.  The outputs are integers in float clothing: every mask comparison is
torch.equal."""
import copy

import numpy as np
import pytest
import torch

import exact_losses as E
import mixmask_ref as R
import multiclass_ref as MR
from test_multiclass import _small_pair, _step_data, _tcfg, fp32_compute  # noqa: F401  (fp32_compute is a fixture)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 19, 33, 64, 4, 5, 8, 9, 16, 17, 32)     # the issue's class counts and the channel-bucket edges
SHAPES = ((17, 31), (7, 9))


def device_classmix(x, keys, dev):
    from ssseg import ops
    mask, present, chosen = ops.classmix_mask(x.to(dev), keys.to(dev), return_state=True)
    torch.cuda.synchronize()
    return mask.cpu(), present.cpu(), chosen.cpu()


def check_classmix(name, x, keys, dev):
    mask, present, chosen = device_classmix(x, keys, dev)
    rmask, rpresent, rchosen, n, k = R.classmix(x, keys)
    print(f'{name}: present {R.fmt_words(present)} / {R.fmt_words(rpresent)} chosen {R.fmt_words(chosen)} / '
          f'{R.fmt_words(rchosen)} n {R.popcounts(present)} / {n} k {R.popcounts(chosen)} / {k} '
          f'mask mean {float(mask.mean()):.4f} / {float(rmask.mean()):.4f} '
          f'differing pixels {int((mask != rmask).sum())}')
    assert torch.equal(present, rpresent) and torch.equal(chosen, rchosen)
    assert R.popcounts(present) == n and R.popcounts(chosen) == k
    assert mask.dtype == torch.float32 and torch.equal(mask, rmask)
    return n


@pytest.mark.parametrize('C', WIDTHS)
def test_classmix_exact(hip_device, C):
    for H, W in SHAPES:
        for dtype in (torch.float32, torch.bfloat16) + ((torch.float16,) if C == 19 else ()):
            x, keys = R.classmix_inputs(C, H, W, dtype)
            n = check_classmix(f'C={C} {H}x{W} {dtype}', x, keys, hip_device)
            assert n[1] == 1                              # image 1: one class, the full mask
            assert n[0] == min(C, H * W)                  # image 0: every class (all but one at C = 64 on 63 pixels)


def test_classmix_no_leak_between_images(hip_device):
    """image 0 holds classes {0,1} only, image 1 {2,3} only; in each image the absent classes have the smallest keys"""
    g = torch.Generator().manual_seed(5)
    lab = torch.stack([torch.randint(0, 2, (17, 31), generator=g), torch.randint(2, 4, (17, 31), generator=g)])
    x = torch.randn(2, 4, 17, 31, generator=g) * 0.1 + 3.0 * torch.nn.functional.one_hot(lab, 4).permute(0, 3, 1, 2)
    keys = torch.tensor([[900, 800, 1, 2], [3, 4, 700, 600]], dtype=torch.int32)
    mask, present, chosen = device_classmix(x, keys, hip_device)
    print('present', R.fmt_words(present), 'chosen', R.fmt_words(chosen))
    assert present.tolist() == [0b0011, 0b1100]
    assert chosen.tolist() == [0b0010, 0b1000]            # k = 1 of n = 2: the smaller key among the PRESENT classes
    check_classmix('no leak', x, keys, hip_device)


def test_classmix_past_the_grid(hip_device):
    """exact_losses.S_GRID = (3, 2, 1, 349 623): 1366 tiles of 256 pixels per image on the 1024 // 3 = 341 workgroups
    per image that the label and write kernels launch: four rounds and a partial fifth"""
    shape = tuple(E.S_GRID)
    assert -(-shape[2] * shape[3] // 256) > 4 * (1024 // shape[0])
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g)
    x[2, 0] = -9.0                                        # image 2: class 1 only, but for its last pixel
    x[2, 1] = 9.0
    x[2, 0, 0, -1] = 10.0
    keys = torch.tensor([[5, 3], [3, 5], [1, 2]], dtype=torch.int32)
    n = check_classmix('S_GRID', x, keys, hip_device)
    assert n == [2, 2, 2]


def test_classmix_strided_logits(hip_device):
    from ssseg import ops
    x, keys = R.classmix_inputs(5, 17, 31)
    ref = R.classmix(x, keys)[0]
    xd, kd = x.to(hip_device), keys.to(hip_device)
    big = torch.zeros(2, 10, 34, 33, device=hip_device)
    big[:, ::2, ::2, 2:] = xd
    views = {'contiguous': xd, 'channels_last': xd.contiguous(memory_format=torch.channels_last),
             'strided view': big[:, ::2, ::2, 2:], 'channel-strided': torch.stack([xd, -xd], 2).flatten(1, 2)[:, ::2]}
    for name, v in views.items():
        assert torch.equal(v.isnan(), xd.isnan()) and torch.equal(v.nan_to_num(), xd.nan_to_num())
        mask = ops.classmix_mask(v, kd).cpu()
        print(name, v.stride(), 'differing pixels', int((mask != ref).sum()))
        assert torch.equal(mask, ref), name


def test_classmix_comparison_can_fail(hip_device):
    """the same comparison fails for a restatement that takes floor(n/2), and for one that ignores presence"""
    lab = torch.tensor([[[0, 1, 2, 0]], [[0, 1, 1, 0]]])
    x = torch.nn.functional.one_hot(lab, 3).permute(0, 3, 1, 2).float()
    keys = torch.tensor([[20, 10, 30], [10, 20, 30]], dtype=torch.int32)
    mask, _, chosen = device_classmix(x, keys, hip_device)
    good = R.classmix(x, keys)
    floor = R.classmix(x, keys, half=lambda n: n // 2)
    blind = R.classmix(x, keys, use_presence=False)
    print('device', mask.flatten().tolist(), 'ceil', good[0].flatten().tolist(), 'floor', floor[0].flatten().tolist(),
          'no presence', blind[0].flatten().tolist())
    assert torch.equal(mask, good[0]) and torch.equal(chosen, good[2])
    assert not torch.equal(mask[0], floor[0][0])          # n = 3: ceil takes 2 classes, floor 1
    assert not torch.equal(mask[1], blind[0][1])          # n = 2 of C = 3: k = 1 class, not the 2 of ceil(3/2)


# (130, 127): 16 510 pixels, past one round of the 64 workgroups x 256 pixels the kernel launches per image
@pytest.mark.parametrize('H,W', ((17, 31), (64, 48), (130, 127)))
def test_cutmix_exact(hip_device, H, W):
    from ssseg import ops
    p, th, tw, tt, tl = R.cutmix_terms(R.DESIGNED, H, W, R.RANGE)
    margin = min(float(R.half_integer_distance(t).min()) for t in (th, tw, tt, tl))
    print('distance of the rounded terms to a half-integer', margin)
    assert margin >= 1e-6                                 # fp64 pow on device and host cannot disagree at a rounding edge
    cases = {'designed': (R.DESIGNED, R.RANGE), 'full': (R.DESIGNED, (1.0, 1.0)), 'empty': (R.DESIGNED, (0.0, 0.0))}
    for name, (params, rng) in cases.items():
        mask, boxes = ops.cutmix_mask(params.to(hip_device), H, W, rng, return_boxes=True)
        rmask, rboxes = R.cutmix(params, H, W, rng)
        print(name, 'boxes', boxes.cpu().tolist(), '/', rboxes.tolist(), 'differing pixels',
              int((mask.cpu() != rmask).sum()))
        assert torch.equal(boxes.cpu(), rboxes)
        assert mask.dtype == torch.float32 and torch.equal(mask.cpu(), rmask)
        assert name != 'full' or bool(mask.all())
        assert name != 'empty' or not bool(mask.any())


def _counter(dev):
    import cowmix
    torch.cuda.synchronize()
    return int(cowmix._DEVICE_RNG['ctr'][dev.index or 0].item())


def test_device_draws(hip_device):
    import mixmasks
    assert mixmasks.DRAW_SOURCE == 'device' and not mixmasks.draws_fixed()
    mixmasks.draw('params', 1, 1, hip_device)             # the counter tensor exists from here on
    for B, C in ((2, 5), (64, 19), (3, 64), (5, 1)):
        c0 = _counter(hip_device)
        k1 = mixmasks.draw('keys', B, C, hip_device)
        c1 = _counter(hip_device)
        k2 = mixmasks.draw('keys', B, C, hip_device)
        p1 = mixmasks.draw('params', B, C, hip_device)
        c3 = _counter(hip_device)
        p2 = mixmasks.draw('params', B, C, hip_device)
        print(f'B={B} C={C}: counter {c0} -> {c1} -> {c3}, documented advance {mixmasks.counter_advance(B, C)}; keys '
              f'[{int(k1.min())}, {int(k1.max())}] params [{float(p1.min())}, {float(p1.max())}]')
        assert c1 - c0 == mixmasks.counter_advance(B, C) == B * (-(-C // 4) + 1) and c3 - c1 == 2 * (c1 - c0)
        assert k1.dtype == torch.int32 and tuple(k1.shape) == (B, C) and bool((k1 >= 0).all())
        assert p1.dtype == torch.float32 and tuple(p1.shape) == (B, 4) and bool((p1 >= 0).all() and (p1 < 1).all())
        assert not torch.equal(k1, k2) and not torch.equal(p1, p2)


def test_device_choice_is_uniform(hip_device):
    """B = 4096 images of 2 x 2 pixels with all 4 classes present: every image has k = 2 chosen and each class is
    chosen with frequency 0.5 +- 0.04 (5 sigma of a fair coin at 4096 draws, sigma = 0.0078)"""
    import mixmasks
    from ssseg import ops
    B = 4096
    x = torch.eye(4).view(1, 4, 2, 2).repeat(B, 1, 1, 1).to(hip_device)
    keys = mixmasks.draw('keys', B, 4, hip_device)
    mask, present, chosen = ops.classmix_mask(x, keys, return_state=True)
    chosen = chosen.cpu()
    freq = [float(((chosen >> c) & 1).float().mean()) for c in range(4)]
    print('chosen frequency per class', freq, 'k', sorted(set(R.popcounts(chosen))))
    assert bool((present.cpu() == 0b1111).all()) and set(R.popcounts(chosen)) == {2}
    assert all(abs(f - 0.5) <= 0.04 for f in freq)
    assert torch.equal(mask.cpu().view(B, 4), torch.stack([(chosen >> c) & 1 for c in range(4)], 1).float())


# ---- the training step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('classmix', 'cutmix'))
def test_step_vs_oracle(hip_device, fp32_compute, monkeypatch, kind):  # noqa: F811
    """three semi-supervised steps of a 5-class SimpleUNet at 64^2, batch 2, epoch 26, softmax consistency, threshold
    0.5 (the step test of tests/test_multiclass.py) with the new mask and host-fixed draws.  The masks the step made are
    recorded with their inputs, each is checked against the restatement, and the oracle's train_epoch is handed the
    recorded masks in order (re-deriving them from the oracle's own teacher would let a near-tie argmax turn an fp
    difference into another mask)."""
    import cowmix
    import mixmasks
    import train
    from oracle import train_ref
    from parity import check_losses
    from ssseg import arena, optim
    C, steps = 5, 3
    student, teacher, ref_s, ref_t = _small_pair(C, hip_device)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps)
    tc = _tcfg('softmax', mix_mask=kind)
    keys = torch.tensor([[40, 10, 30, 20, 50], [5, 4, 3, 2, 1]], dtype=torch.int32)
    params = R.DESIGNED[[0, 7]]
    margin = min(float(R.half_integer_distance(t).min())
                 for t in R.cutmix_terms(params, 64, 64, tc['mask_proportion_range'])[1:])
    print('distance of the rounded box terms to a half-integer', margin)
    assert margin >= 1e-6
    seen = []
    name = f'generate_{kind}_masks_like'
    real = getattr(mixmasks, name)

    def recording(example, *a, **kw):
        m = real(example, *a, **kw)
        seen.append((example.detach().float().cpu(), m.detach().float().cpu()))
        return m
    monkeypatch.setattr(mixmasks, name, recording)
    monkeypatch.setattr(cowmix, 'generate_cowmix_masks_like', None)        # the step must not take the CowMix path
    mixmasks.set_draws(keys=keys, params=params)
    try:
        assert train._graph_key(student, teacher, opt, imgs[0].to(hip_device), masks[0].to(hip_device),
                                unl[0].to(hip_device), unl[1].to(hip_device), 26, 5, {'train': tc}) is None
        student.train()
        opt.zero_grad()
        logs = []
        for k in range(steps):
            c, u, cm = train.train_step(student, teacher, opt, imgs[k].to(hip_device), masks[k].to(hip_device),
                                        unl[2 * k].to(hip_device), unl[2 * k + 1].to(hip_device), 26, k, {'train': tc})
            logs.append((float(c), float(u)))
            print(f'step {k}: sup {float(c)!r} unsup {float(u)!r} cm {float(cm)!r}')
    finally:
        mixmasks.set_draws()
    assert len(seen) == steps
    for k, (example, m) in enumerate(seen):
        if kind == 'classmix':
            ref, _, _, n, kk = R.classmix(example, keys)
            print(f'step {k}: n {n} k {kk} mask mean {float(m.mean()):.4f} differing pixels {int((m != ref).sum())}')
        else:
            ref, boxes = R.cutmix(params, 64, 64, tc['mask_proportion_range'])
            print(f'step {k}: boxes {boxes.tolist()} mask mean {float(m.mean()):.4f} differing pixels '
                  f'{int((m != ref).sum())}')
        assert tuple(m.shape) == (2, 1, 64, 64) and torch.equal(m, ref)
    assert any(0 < float(m.mean()) < 1 for _, m in seen)                   # a mask that mixes something

    monkeypatch.setattr(train_ref, 'consistency_loss', lambda s, t, thr: MR.consistency_softmax(s, t, thr)[:2])

    def oracle(dt):
        s, t = copy.deepcopy(ref_s).to(dt), copy.deepcopy(ref_t).to(dt)
        o = torch.optim.SGD(s.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        recorded = iter([m for _, m in seen])
        monkeypatch.setattr(train_ref, 'cowmix_mask_like', lambda ex, *a, **kw: next(recorded).to(ex.dtype))
        return train_ref.train_epoch(s, t, o, list(zip(imgs.to(dt), masks.to(dt))), iter(unl.to(dt)), 26,
                                     train_ref.default_cfg(sigma_range=(2, 4), confidence_threshold=0.5))
    r32, r64 = oracle(torch.float32), oracle(torch.float64)
    print('oracle fp64:', r64)
    assert all(0.02 < r['cm_mean'] < 0.98 and r['unsup_loss'] > 0 for r in r64)   # the gate is open
    check_losses(logs, [(r['sup_loss'], r['unsup_loss']) for r in r32],
                 [(r['sup_loss'], r['unsup_loss']) for r in r64])


def _device_steps(dev, tc, graphed=False, steps=3, same_inputs=False):
    """2 eager steps + `steps` more (eager, or replays of one captured step), every draw on the device, the counters
    reset first.  Returns (losses, state, Philox counter at the end)."""
    import cowmix
    import mixmasks
    import train
    from ssseg import arena, optim
    from ssseg.graph import StepGraph
    C = 5
    student, teacher, _, _ = _small_pair(C, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps + 2)
    data = [(imgs[k].to(dev), masks[k].to(dev), unl[2 * k].to(dev), unl[2 * k + 1].to(dev)) for k in range(steps + 2)]
    if same_inputs:
        data[3:] = [data[2]] * (steps - 1)
    cfg = {'train': tc}
    assert cowmix.NOISE_SOURCE == 'device' and mixmasks.DRAW_SOURCE == 'device' and not mixmasks.draws_fixed()
    mixmasks.draw('params', 1, 1, dev)                    # the counter tensor exists from here on
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    student.train()
    opt.zero_grad()
    out = [train.train_step(student, teacher, opt, *data[k], 26, k, cfg) for k in range(2)]
    if graphed:
        assert train._graph_key(student, teacher, opt, *data[2], 26, 2, cfg) is not None
        g = StepGraph(lambda i, m, a, b: train.train_step(student, teacher, opt, i, m, a, b, 26, 2, cfg), *data[2])
        for k in range(2, steps + 2):
            out.append(tuple(t.clone() for t in g(*data[k])))
    else:
        for k in range(2, steps + 2):
            out.append(train.train_step(student, teacher, opt, *data[k], 26, k, cfg))
    torch.cuda.synchronize()
    state = {**{'s.' + k: v.detach().clone() for k, v in student.state_dict().items()},
             **{'t.' + k: v.detach().clone() for k, v in teacher.state_dict().items()}}
    return [tuple(float(t) for t in l) for l in out], state, _counter(dev)


@pytest.mark.parametrize('kind', ('classmix', 'cutmix'))
def test_graph_replay_matches_eager_bitwise_with_fresh_draws(hip_device, fp32_compute, kind):  # noqa: F811
    import mixmasks
    eager, s_e, c_e = _device_steps(hip_device, _tcfg('softmax', mix_mask=kind))
    graph, s_g, c_g = _device_steps(hip_device, _tcfg('softmax', mix_mask=kind), graphed=True)
    per_step = mixmasks.counter_advance(2, 5 if kind == 'classmix' else 1)
    print('eager', eager, 'graph', graph, 'counter', c_e, c_g, 'documented', 5 * per_step)
    assert np.array_equal(np.array(eager), np.array(graph), equal_nan=True)
    assert all(np.isfinite(l).all() and l[1] > 0 and 0 < l[2] < 1 for l in eager)
    assert c_e == c_g == 5 * per_step                     # every step, eager or replayed, drew from the counter
    for k in s_e:
        assert torch.equal(s_e[k], s_g[k]), k
    same, _, c_s = _device_steps(hip_device, _tcfg('softmax', mix_mask=kind), graphed=True, steps=2, same_inputs=True)
    print('two replays on the same inputs', same[2:], 'counter', c_s)
    assert same[2][1] != same[3][1] and c_s == 4 * per_step


def test_default_and_cowmix_key_are_the_same_path(hip_device, fp32_compute):  # noqa: F811
    """a config without mix_mask and one with mix_mask='cowmix': identical bits, the counter at the same value"""
    import train
    none, s_n, c_n = _device_steps(hip_device, _tcfg('softmax'), steps=1)
    cow, s_c, c_c = _device_steps(hip_device, _tcfg('softmax', mix_mask='cowmix'), steps=1)
    cut, _, c_u = _device_steps(hip_device, _tcfg('softmax', mix_mask='cutmix'), steps=1)
    print('no key', none, 'cowmix', cow, 'cutmix', cut, 'counters', c_n, c_c, c_u)
    assert none == cow and c_n == c_c == 3 * (2 + 2 * 64 * 64 // 4 + 1)     # CowMix's B + ceil(B HW / 4) + 1 per step
    assert all(torch.equal(s_n[k], s_c[k]) for k in s_n)
    assert c_u != c_n and all(a[1] != b[1] for a, b in zip(none, cut))      # another mask is another loss
    with pytest.raises(ValueError, match='mix_mask'):
        train._teacher_targets(None, None, None, {'mix_mask': 'fmix'})
