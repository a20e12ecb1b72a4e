"""Geometric consistency on the device: the per-sample affine warp (ssseg_affine_warp_fwd / _bwd), its validity map,
the device draw, the weighted consistency loss and the wiring into the training step, each against the fp64
restatement of tests/geo_ref.py.

Tolerance of the warp (BOUND below): 16 * 2^-23 * max(H, W) * (max x - min x).  Each sampling coordinate carries at
most 4 fp32 roundings of magnitude <= max(H, W) (the rounded matrix entries and the two fmaf), there are two
coordinates, and bilinear interpolation changes by at most the data range per pixel of coordinate error; a wrong tap or
a shifted centre errs by 0.1 or more on these inputs."""
import pytest
import torch

import geo_ref
import philox_ref
from geo_ref import PAIRS

pytestmark = pytest.mark.gpu

# (shape, per-sample (theta, s)): every pair of geo_ref.PAIRS, mixed within the batches; (2,2,64,64) is more pixels
# than the threads of one 256-thread block times its channel lanes
CASES = [((2, 3, 19, 24), [PAIRS[0], PAIRS[1]]), ((2, 3, 19, 24), [PAIRS[2], PAIRS[3]]),
         ((1, 1, 5, 7), [PAIRS[4]]), ((1, 1, 5, 7), [PAIRS[5]]),
         ((2, 2, 33, 70), [PAIRS[6], PAIRS[7]]), ((2, 2, 33, 70), [PAIRS[3], PAIRS[0]]),
         ((1, 2, 1, 9), [PAIRS[1]]), ((1, 2, 1, 9), [PAIRS[0]]),
         ((2, 2, 64, 64), [PAIRS[5], PAIRS[4]]), ((2, 2, 64, 64), [PAIRS[2], PAIRS[1]])]
IDS = [f'{"x".join(map(str, s))}-{"_".join(str(p[0]) for p in ps)}' for s, ps in CASES]


def _bound(H, W, rng=1.0):
    return 16 * 2.0 ** -23 * max(H, W) * rng


def _data(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64), torch.randn(*shape, generator=g, dtype=torch.float64)


def _mats(params, H, W, dev):
    from ssseg import ops
    return ops.affine_mats([p[0] for p in params], [p[1] for p in params], H, W, dev)


def _n_box(inv):
    """pixels of the backward's search box: half-extents |ia|+|ib|+1 and |ic|+|id|+1"""
    ex = inv[:, 0].abs() + inv[:, 1].abs() + 1
    ey = inv[:, 3].abs() + inv[:, 4].abs() + 1
    return float(((2 * ex).floor() + 1).max() * ((2 * ey).floor() + 1).max())


@pytest.mark.parametrize('shape,params', CASES, ids=IDS)
def test_forward_vs_fp64(hip_device, shape, params):
    from ssseg import ops
    B, C, H, W = shape
    x, _ = _data(shape)
    m64, _ = geo_ref.mats64(params, H, W)
    ref = geo_ref.warp(x, m64)
    mats, inv = _mats(params, H, W, hip_device)
    xd = x.float().to(hip_device)
    y = ops.affine_warp(xd, mats, inv)
    err = float((y.cpu().double() - ref).abs().max())
    print(f'forward {shape} {params}: err {err:.3e} bound {_bound(H, W):.3e}')
    assert err <= _bound(H, W, float(x.max() - x.min()))
    for b, (theta, s) in enumerate(params):
        if (theta, s) == (0.0, 1.0):
            assert torch.equal(y[b], xd[b])                 # the identity sample: bit for bit
        if s == 1.0:
            rot = ops.rotate(xd[b:b + 1], theta)
            assert float((y[b:b + 1] - rot).abs().max()) <= _bound(H, W)


@pytest.mark.parametrize('shape,params', CASES, ids=IDS)
def test_backward_vs_fp64_autograd(hip_device, shape, params):
    from ssseg import ops
    B, C, H, W = shape
    x, gy = _data(shape)
    m64, i64 = geo_ref.mats64(params, H, W)
    xr = x.clone().requires_grad_(True)
    geo_ref.warp(xr, m64).backward(gy)
    mats, inv = _mats(params, H, W, hip_device)
    grads = []
    for _ in range(2):
        xd = x.float().to(hip_device).requires_grad_(True)
        ops.affine_warp(xd, mats, inv).backward(gy.float().to(hip_device))
        grads.append(xd.grad)
    assert torch.equal(grads[0], grads[1])                  # a gather: the same bits on every run
    bound = _bound(H, W) * float(gy.abs().max()) * _n_box(i64)
    err = float((grads[0].cpu().double() - xr.grad).abs().max())
    print(f'backward {shape} {params}: err {err:.3e} bound {bound:.3e}')
    assert err <= bound
    # <warp(x), g> = <x, warp_bwd(g)> (positive g: a well-conditioned sum), both sums in fp64
    g = (gy.abs() + 0.5).float().to(hip_device)
    xd = x.float().to(hip_device).requires_grad_(True)
    y = ops.affine_warp(xd, mats, inv)
    y.backward(g)
    lhs = float((y.detach().double() * g.double()).sum())
    rhs = float((xd.detach().double() * xd.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('shape,params', CASES, ids=IDS)
def test_16bit_and_channels_last(hip_device, shape, params, dtype):
    from ssseg import ops
    B, C, H, W = shape
    x, gy = _data(shape)
    mats, inv = _mats(params, H, W, hip_device)
    rnd = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    x16, g16 = x.to(dtype).to(hip_device), gy.to(dtype).to(hip_device)
    out = {}
    for name, fmt in (('nchw', torch.contiguous_format), ('nhwc', torch.channels_last)):
        xd = x16.clone(memory_format=fmt).requires_grad_(True)
        y = ops.affine_warp(xd, mats, inv)
        y.backward(g16.contiguous(memory_format=fmt))
        assert y.dtype == dtype and xd.grad.dtype == dtype
        out[name] = (y.detach(), xd.grad)
    assert torch.equal(out['nchw'][0], out['nhwc'][0])      # the two layouts agree bitwise
    assert torch.equal(out['nchw'][1], out['nhwc'][1])
    # against the fp32 kernel on the same rounded values: one output rounding plus the fp32 bound
    x32 = x16.float().requires_grad_(True)
    y32 = ops.affine_warp(x32, mats, inv)
    y32.backward(g16.float())
    y32 = y32.detach()
    assert bool(((out['nchw'][0].float() - y32).abs() <= rnd * y32.abs() + _bound(H, W)).all())
    gb = _bound(H, W) * float(gy.abs().max()) * _n_box(inv.cpu().double())
    assert bool(((out['nchw'][1].float() - x32.grad).abs() <= rnd * x32.grad.abs() + gb).all())


@pytest.mark.parametrize('hw', [(19, 24), (33, 70)], ids=['19x24', '33x70'])
def test_validity_map_exact(hip_device, hw):
    from ssseg import ops
    H, W = hw
    params = [PAIRS[1], PAIRS[2], PAIRS[3], PAIRS[5], PAIRS[7]]
    m64, i64 = geo_ref.mats64(params, H, W)
    # no sampling coordinate comes near a border of the rule, so fp32 and fp64 decide every pixel alike
    assert geo_ref.border_clearance(m64, H, W) > 1e-3 and geo_ref.border_clearance(i64, H, W) > 1e-3
    mats, inv = _mats(params, H, W, hip_device)
    x = torch.rand(len(params), 1, H, W, device=hip_device)
    _, v = ops.affine_warp(x, mats, inv, want_valid=True)
    _, vi = ops.affine_warp(x, inv, mats, want_valid=True)
    assert v.dtype == torch.float32 and tuple(v.shape) == (len(params), H, W)
    assert torch.equal(v.cpu().double(), geo_ref.valid(m64, H, W))
    assert torch.equal(vi.cpu().double(), geo_ref.valid(i64, H, W))
    assert 0 < float(v.mean()) < 1 and 0 < float(vi.mean()) < 1
    ident, _ = _mats([PAIRS[0]], H, W, hip_device)
    _, v1 = ops.affine_warp(x[:1], ident, ident, want_valid=True)
    assert torch.equal(v1, torch.ones_like(v1))


def test_weighted_consistency_vs_fp64(hip_device):
    import numpy as np
    from ssseg import ops
    g = torch.Generator().manual_seed(11)
    s = torch.randn(2, 2, 19, 24, generator=g) * 2
    t = torch.randn(2, 2, 19, 24, generator=g) * 2
    w = (torch.rand(2, 19, 24, generator=g) > 0.3).float() * torch.rand(2, 19, 24, generator=g)
    thr = 0.7
    assert geo_ref.gate_clearance(t, thr) > 1e-5            # no pixel's gate hangs on an fp32 rounding
    sr = s.double().requires_grad_(True)
    ref, ref_cm = geo_ref.consistency_w(sr, t, w, thr)
    (ref * 10.0).backward()
    sd = s.to(hip_device).requires_grad_(True)
    loss, cm = ops.consistency_loss_weighted(sd, t.to(hip_device), w.to(hip_device), thr)
    (loss * 10.0).backward()
    np.testing.assert_allclose(float(loss.detach()) * 10.0, float(ref.detach()) * 10.0, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(float(cm.detach()), float(ref_cm.detach()), rtol=2e-5)
    np.testing.assert_allclose(sd.grad.cpu().numpy(), sr.grad.float().numpy(), rtol=2e-4, atol=2e-8)
    # w == 1: the unweighted entry points' bits
    one = torch.ones(2, 19, 24, device=hip_device)
    s1 = s.to(hip_device).requires_grad_(True)
    s2 = s.to(hip_device).requires_grad_(True)
    l1, c1 = ops.consistency_loss_weighted(s1, t.to(hip_device), one, thr)
    l2, c2 = ops.consistency_loss(s2, t.to(hip_device), thr)
    l1.backward()
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(c1, c2) and torch.equal(s1.grad, s2.grad)
    # w == 0: 0/0
    l0, c0 = ops.consistency_loss_weighted(s.to(hip_device), t.to(hip_device), torch.zeros_like(one), thr)
    assert bool(torch.isnan(l0)) and float(c0) == 0.0


def test_device_draw(hip_device):
    import cowmix
    import reversible_augmentations as RA
    B, H, W = 64, 24, 32
    aug = RA.RotateRescale(15, 0.75, 1.25)
    x = torch.zeros(B, 1, H, W, device=hip_device)
    aug._draw(x[:1])                                        # creates the device counter if this is its first use
    ctr = cowmix._DEVICE_RNG['ctr'][hip_device.index]
    ctr.fill_(1000)
    mats, inv = aug._draw(x)
    assert int(ctr) == 1000 + B                             # the documented advance: B
    m, mi = mats.cpu().double(), inv.cpu().double()
    # A = [al, be, ..; -be, al, ..] with al = cos/s, be = -sin/s: recover (theta, s); fp32 entries, so 1e-5 of slack
    s = 1.0 / torch.sqrt(m[:, 0] ** 2 + m[:, 1] ** 2)
    theta = torch.rad2deg(torch.atan2(-m[:, 1], m[:, 0]))
    assert float(theta.abs().max()) <= 15 + 1e-5 and float(s.min()) >= 0.75 - 1e-5 and float(s.max()) <= 1.25 + 1e-5
    assert float(theta.max()) > 5 and float(theta.min()) < -5 and float(s.max()) > 1.1 and float(s.min()) < 0.9
    assert torch.equal(m[:, 3], -m[:, 1]) and torch.equal(m[:, 4], m[:, 0])
    assert len({tuple(r.tolist()) for r in mats.cpu()}) == B          # the samples of a batch are distinct
    # the reference is drawn, not recovered from the matrices under test: theta and s from the host Philox restatement
    # at this seed and counter (tests/philox_ref.py, stream 2), the matrices within the bounds derived there
    _, _, ref, ref_inv = philox_ref.affine_draw(B, H, W, 15, 0.75, 1.25, cowmix._DEVICE_RNG['seed'], 1000)
    philox_ref.check_affine(mats.cpu().numpy(), ref, H, W, 'A')
    philox_ref.check_affine(inv.cpu().numpy(), ref_inv, H, W, 'A^-1')
    row = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    for a, b in zip(m, mi):
        prod = torch.cat([a.reshape(2, 3), row]) @ torch.cat([b.reshape(2, 3), row])
        assert float((prod - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5
    mats2, inv2 = aug._draw(x)                              # the advanced counter: other draws
    assert not torch.equal(mats2, mats) and int(ctr) == 1000 + 2 * B
    ctr.fill_(1000)
    mats3, inv3 = aug._draw(x)                              # the same seed and counter: the same bits
    assert torch.equal(mats3, mats) and torch.equal(inv3, inv)


def _steps(device, aug=None, graphed=False, steps=3, size=64, batch=2, again=False):
    """the pattern of tests/test_graph.py: two eager steps, then `steps` more, eager or replayed from one capture"""
    import bench
    import cowmix
    import train
    from ssseg.graph import StepGraph
    model, teacher, opt, cfg = bench.build(batch, size, device)
    if aug is not None:
        cfg['train']['consistency_augmentation'] = aug
    data = bench.synthetic_batches(steps + 2, batch, size, device, 0)
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    model.train()
    opt.zero_grad()
    losses = [train.train_step(model, teacher, opt, *data[k], 30, k, cfg) for k in range(2)]
    extra = []
    if graphed:
        g = StepGraph(lambda i, m, a, b: train.train_step(model, teacher, opt, i, m, a, b, 30, 2, cfg), *data[2])
        for k in range(2, steps + 2):
            losses.append(tuple(t.clone() for t in g(*data[k])))
    else:
        for k in range(2, steps + 2):
            losses.append(train.train_step(model, teacher, opt, *data[k], 30, k, cfg))
    torch.cuda.synchronize()
    state = {**{'s.' + k: v.detach().clone() for k, v in model.state_dict().items()},
             **{'t.' + k: v.detach().clone() for k, v in teacher.state_dict().items()}}
    if graphed and again:
        for _ in range(2):                                  # two more replays, both on the SAME inputs
            out = g(*data[2])
            extra.append((float(out[1]), aug.mats.clone()))
    return [tuple(float(t) for t in l) for l in losses], state, extra


def test_wiring_identity_view_is_bitwise_the_plain_step(hip_device):
    """RotateRescale(0, 1, 1): the identity warp and an all-ones validity map must not move a bit of three bf16 steps.
    Its parameters come from the CPU generator (which nothing else in the step reads): the device source would
    advance the Philox counter it shares with CowMix and so change the following steps' masks."""
    import reversible_augmentations as RA
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.bfloat16)
    plain, s_p, _ = _steps(hip_device, steps=1)
    geo, s_g, _ = _steps(hip_device, aug=RA.RotateRescale(0, 1, 1, source='cpu'), steps=1)
    assert plain == geo, (plain, geo)
    assert all(torch.isfinite(torch.tensor(l)).all() for l in plain)
    for k in s_p:
        assert torch.equal(s_p[k], s_g[k]), k


def test_wiring_values_vs_fp64(hip_device, monkeypatch):
    """The step's consistency loss and cm under fixed views equal the fp64 restatement (warp back, validity map,
    gated MSE) fed with the student's resized view logits and the teacher target of the same step."""
    import numpy as np
    import bench
    import reversible_augmentations as RA
    import train
    from ssseg import nn as snn
    from ssseg import ops
    snn.set_compute_dtype(torch.bfloat16)
    params = [PAIRS[1], PAIRS[7]]
    aug = RA.RotateRescale(20, 0.75, 1.25)
    aug.set_params([p[0] for p in params], [p[1] for p in params])
    seen = {}
    reverse, weighted = aug.reverse, ops.consistency_loss_weighted

    def rec_reverse(inputs):
        seen['view_logits'] = inputs[0].detach().float().cpu()
        return reverse(inputs)

    def rec_weighted(s, t, w, thr):
        seen['target'], seen['thr'] = t.detach().float().cpu(), thr
        return weighted(s, t, w, thr)
    monkeypatch.setattr(aug, 'reverse', rec_reverse)
    monkeypatch.setattr(ops, 'consistency_loss_weighted', rec_weighted)
    model, teacher, opt, cfg = bench.build(2, 64, hip_device)
    cfg['train']['consistency_augmentation'] = aug
    # the freshly initialised teacher's logits are ~1e-3, so its confidences crowd around 0.5 (8192 of them within
    # 2e-3): at bench's threshold of 0.5 some gate would hang on the last bit of the fp32 sigmoid, which an fp64
    # restatement cannot decide.  Below that band every pixel is confident (asserted), and the weight that remains is
    # the validity map this test is about; gate x weight is test_weighted_consistency_vs_fp64's ground.
    cfg['train']['confidence_threshold'] = 0.3
    data = bench.synthetic_batches(1, 2, 64, hip_device, 0)
    model.train()
    opt.zero_grad()
    _, unsup, cm = train.train_step(model, teacher, opt, *data[0], 30, 0, cfg)
    H = W = 64
    assert tuple(seen['view_logits'].shape[2:]) == (H, W)
    m64, i64 = geo_ref.mats64(params, H, W)
    assert geo_ref.border_clearance(i64, H, W) > 1e-3
    assert geo_ref.gate_clearance(seen['target'], seen['thr']) > 1e-5
    back = geo_ref.warp(seen['view_logits'].double(), i64)
    ref, ref_cm = geo_ref.consistency_w(back, seen['target'], geo_ref.valid(i64, H, W), seen['thr'])
    weight = float(cfg['train']['consistency_loss_weight'])
    np.testing.assert_allclose(float(unsup), float(ref) * weight, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(float(cm), float(ref_cm), rtol=2e-5)
    assert 0 < float(ref_cm) < 1


def test_graph_key_runs_host_drawn_views_eagerly(hip_device, monkeypatch):
    """views drawn on the device are captured; views drawn or fixed on the host would be repeated by a replay"""
    import types
    import cowmix
    import reversible_augmentations as RA
    import train
    monkeypatch.setattr(cowmix, 'NOISE_SOURCE', 'device')
    monkeypatch.setitem(train._GRAPH, 'on', True)
    model = ema = torch.nn.Identity()
    opt = types.SimpleNamespace(param_groups=[{'lr': 0.1}])
    x = torch.zeros(2, 3, 8, 8, device=hip_device)
    monkeypatch.setitem(train._OVERLAP['seen'], train._step_key(model, ema, x, x), train._GRAPH['eager_steps'])

    def key(aug):
        cfg = {'train': {'use_semi_supervised': True, 'virtual_batch_size_multiplier': 1}}
        if aug is not None:
            cfg['train']['consistency_augmentation'] = aug
        return train._graph_key(model, ema, opt, x, x, x, x, 30, 2, cfg)
    assert key(None) is not None
    assert key(RA.RotateRescale(15, 0.75, 1.25)) is not None
    assert key(lambda: RA.RotateRescale(15, 0.75, 1.25)) is not None
    assert key(RA.RotateRescale(15, 0.75, 1.25, source='cpu')) is None
    fixed = RA.RotateRescale(15, 0.75, 1.25)
    fixed.set_params([1.0, 2.0], [1.0, 1.1])
    assert key(fixed) is None


def test_captured_step_replays_fresh_views_bitwise(hip_device):
    import reversible_augmentations as RA
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.bfloat16)
    eager, s_e, _ = _steps(hip_device, aug=RA.RotateRescale(15, 0.75, 1.25))
    graph, s_g, extra = _steps(hip_device, aug=RA.RotateRescale(15, 0.75, 1.25), graphed=True, again=True)
    assert eager == graph, (eager, graph)
    assert all(torch.isfinite(torch.tensor(l)).all() for l in eager)
    for k in s_e:
        assert torch.equal(s_e[k], s_g[k]), k
    assert extra[0][0] != extra[1][0]                      # two replays on the same inputs: other consistency losses
    assert not torch.equal(extra[0][1], extra[1][1])        # because the views were drawn afresh
