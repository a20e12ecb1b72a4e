"""The residual join's ReLU backward and shortcut-gradient add in the consumer's input-gradient epilogue
(ssseg_conv_igemm_epi_join, snn.set_bn_join).

A ResNet Bottleneck without downsample builds z = relu(bn3(conv3(..)) + z_prev); the next block's conv1 and identity
shortcut are z's only readers and their gradients meet in that conv1's input-gradient launch (GradHandoff).  Its epilogue
adds the shortcut gradient and applies the join's ReLU backward, so what it stores is z's complete masked gradient:
bn3's backward takes it as dy and as the shortcut gradient -- it reads no residual (from which it rebuilt the mask in
both of its passes) and writes no second output.

The second stage of that fusion (bn3's backward sums and the eval BN's scaled gradient from the same epilogue) was built,
measured and rejected: bn3's reduction / eval pass still runs for every join, so these tests
check the stored masked gradient, which launches take the join form, and what the BN kernels are no longer handed."""
import contextlib

import pytest
import torch

from test_hip_layers import ALL_VARIANTS, _act_in, _close, _q, mode  # noqa: F401  (mode: the dtype fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(9, 7), (16, 16)]   # N = 2: M = 126 (partial tiles, W % 16 != 0) and M = 512


def _variants(mode):
    return [0] if mode != 'bf16' else ALL_VARIANTS


def _act_rand(shape, seed, mode, dev, relu=False):
    from ssseg import nn as snn
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    if relu:
        t = t.clamp_min(0.0)
    return snn.to_act(_q(t, mode).to(dev))


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('cin,cout', [(64, 16), (256, 64)])
def test_join_epilogue_engine(hip_device, mode, cin, cout, H, W):
    """(a) A 1x1 conv's input gradient with addend and mask: contraction 16 -> 64 outputs (general-k loader) and
    64 -> 256 (64-channel LDS-DMA path, four n-tiles).  The stored masked gradient equals ssseg_act_bwd(residual-epilogue
    dgrad) bit for bit, on every engine variant."""
    from ssseg import native as N
    from ssseg import nn as snn
    torch.manual_seed(21)
    conv = snn.Conv2d(cin, cout, 1, bias=False).to(hip_device)
    n = 2
    gy = _act_rand((n, cout, H, W), 22, mode, hip_device)
    z = _act_rand((n, cin, H, W), 23, mode, hip_device, relu=True)
    add = _act_rand((n, cin, H, W), 24, mode, hip_device)
    assert z.shape[1] == cin and float((z == 0).float().mean()) > 0.2
    dt = N.dt_code(z)

    # unfused: dgrad + addend (the residual epilogue), then the ReLU backward
    d_ref = conv._ssseg_dgrad(gy, z.shape, residual=add)
    m_ref = torch.empty_like(d_ref)
    N.call('ssseg_act_bwd', N.dev_ptr(d_ref), N.dev_ptr(z), N.dev_ptr(m_ref), d_ref.numel(), snn.ACT_RELU, 0.0, dt,
           N.stream())
    assert float((m_ref != 0).float().mean()) > 0.2
    try:
        for v in _variants(mode):
            N.call('ssseg_set_knob', 4, v)
            dx = conv._ssseg_dgrad(gy, z.shape, residual=add, join=z)
            torch.cuda.synchronize()
            assert dx.__dict__.get('_ssseg_premasked', False), f'variant {v}: the engine declined the join epilogue'
            assert torch.equal(dx, m_ref), f'variant {v}: masked gradient'
    finally:
        N.call('ssseg_set_knob', 4, 0)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_join_epilogue_split_k_tail(hip_device, dtype, H, W):
    """The join epilogue behind the deterministic split-K tail: a 1x1 input gradient contracting 128 channels (two
    k-tiles) with the split forced to S = 2 (knob 14), so the last-arriving slice sums the partials and then runs the
    epilogue.  Bit for bit ssseg_act_bwd of the same split launch with the residual epilogue, on every variant."""
    from ssseg import native as N
    from ssseg import nn as snn
    mode = 'bf16' if dtype == torch.bfloat16 else 'f16'
    snn.set_compute_dtype(dtype)
    try:
        N.call('ssseg_set_knob', 14, 2)
        torch.manual_seed(27)
        conv = snn.Conv2d(256, 128, 1, bias=False).to(hip_device)
        gy = _act_rand((2, 128, H, W), 28, mode, hip_device)
        z = _act_rand((2, 256, H, W), 29, mode, hip_device, relu=True)
        add = _act_rand((2, 256, H, W), 30, mode, hip_device)
        d = snn._desc(N=2, H=H, W=W, C=128, ldx=128, OH=H, OW=W, K=256, R=1, S=1, sy=1, sx=1, dy=1, dx=1, py=0, px=0,
                      outH=H, outW=W, osy=1, osx=1, ooy=0, oox=0, ldy=256, ldw=128)
        assert N.lib().ssseg_conv_igemm_workspace_bytes(snn.ctypes_ref(d), N.dt_code(z)) > 0   # the launch splits
        d_ref = conv._ssseg_dgrad(gy, z.shape, residual=add)
        m_ref = torch.empty_like(d_ref)
        N.call('ssseg_act_bwd', N.dev_ptr(d_ref), N.dev_ptr(z), N.dev_ptr(m_ref), d_ref.numel(), snn.ACT_RELU, 0.0,
               N.dt_code(z), N.stream())
        for v in _variants(mode):
            N.call('ssseg_set_knob', 4, v)
            dx = conv._ssseg_dgrad(gy, z.shape, residual=add, join=z)
            torch.cuda.synchronize()
            assert dx.__dict__.get('_ssseg_premasked', False), f'variant {v}: the engine declined the join epilogue'
            assert torch.equal(dx, m_ref), f'variant {v}: masked gradient'
    finally:
        N.call('ssseg_set_knob', 4, 0)
        N.call('ssseg_set_knob', 14, 0)
        snn.set_compute_dtype(torch.bfloat16)


def _stack(inplanes, width, dev, ill=False):
    from models.encoders.resnet import Bottleneck
    torch.manual_seed(31)
    blocks = [Bottleneck(inplanes, width) for _ in range(3)]
    for b in blocks[:-1]:
        b.join_use = True
    net = torch.nn.Sequential(*blocks).to(dev)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.num_features, generator=g) * 0.6 - 0.3)
                m.running_mean.copy_(torch.rand(m.num_features, generator=g) * 0.4 - 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
        if ill:   # bn3 channels the y-based x_hat could not resolve: gamma 0 / 1e-3 with |beta| = 1
            for b in blocks:
                b.bn3.weight[0::4] = 0.0
                b.bn3.weight[1::4] = 1e-3
                b.bn3.bias[0::4] = 1.0   # (+1: the join's ReLU stays open there, so the true dgamma is not 0)
                b.bn3.bias[1::4] = 1.0
    return net


def _names(net):
    return ['dx'] + [k for k, _ in net.named_parameters()]


def _run_stack(net, x, g, kind, dev):
    from ssseg import nn as snn
    net.train(kind == 'train')
    net.zero_grad(set_to_none=True)
    xa = _act_in(x, dev).detach().requires_grad_(True)
    y = net(xa)
    with (snn.defer_param_grads() if kind == 'eval_deferred' else contextlib.nullcontext()):
        y.backward(snn.to_act(g.to(dev)))
    torch.cuda.synchronize()
    return [xa.grad.float().cpu()] + [p.grad.float().cpu().clone() for p in net.parameters()]


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('kind,ill', [('train', False), ('train', True), ('eval_deferred', False),
                                      ('eval_immediate', False), ('eval_immediate', True)])
@pytest.mark.parametrize('inplanes,width', [(64, 16), (256, 64)])
def test_bottleneck_stack_join(hip_device, mode, monkeypatch, inplanes, width, kind, ill, H, W):
    """(b) Three Bottlenecks without downsample, the first two declared join_use: with the switch on the second and
    third block's conv1 input gradients run the join epilogue, the first two bn3 backwards are handed no residual and
    asked for no shortcut gradient, and the input gradient, every weight gradient and every dgamma / dbeta agree with
    the switch-off run -- per channel on bn3 channels with gamma in {0, 1e-3} and |beta| = 1."""
    from ssseg import native as N
    from ssseg import nn as snn
    net = _stack(inplanes, width, hip_device, ill)
    x = _q(torch.randn(2, inplanes, H, W, generator=torch.Generator().manual_seed(33)), mode)
    g = _q(torch.randn(2, inplanes, H, W, generator=torch.Generator().manual_seed(34)), mode)
    calls = []
    real, real_u = N.call, N.call_or_unsupported

    def spy(name, *a):
        calls.append((name, a))
        return real(name, *a)

    def spy_u(name, *a):
        calls.append((name, a))
        return real_u(name, *a)

    monkeypatch.setattr(N, 'call', spy)
    monkeypatch.setattr(N, 'call_or_unsupported', spy_u)

    def count():
        """(join launches, bn3 backward passes handed a residual or asked for a shortcut gradient)"""
        joins = sum(1 for c, _ in calls if c == 'ssseg_conv_igemm_epi_join')
        if kind == 'train':   # ssseg_bn_bwd_reduce_grad(dy, x, residual, ..), ssseg_bn_bwd_apply(dy, x, residual, dx, dres, ..)
            heavy = sum(1 for c, a in calls if (c == 'ssseg_bn_bwd_reduce_grad' and a[2] is not None)
                        or (c == 'ssseg_bn_bwd_apply' and (a[2] is not None or a[4] is not None)))
            return joins, heavy
        # ssseg_bn_eval_bwd_part / _grad(dy, y, aux, dconv, dres, ..)
        return joins, sum(1 for c, a in calls if c in ('ssseg_bn_eval_bwd_part', 'ssseg_bn_eval_bwd_grad')
                          and a[4] is not None)

    names = _names(net)
    try:
        for v in _variants(mode):
            # the switch-off run of the same variant: forcing a variant changes every conv of the stack, and a stack of
            # training-mode BNs over 126 / 512 pixels amplifies rounding-level differences far beyond the join's own
            N.call('ssseg_set_knob', 4, v)
            snn.set_bn_join(False)
            calls.clear()
            ref = _run_stack(net, x, g, kind, hip_device)
            assert count() == (0, 6 if kind == 'train' else 3), (v, count())
            snn.set_bn_join(True)
            calls.clear()
            got = _run_stack(net, x, g, kind, hip_device)
            assert count() == (2, 2 if kind == 'train' else 1), (v, count())
            for a, b, what in zip(got, ref, names):
                _close(a, b, mode, f'variant {v} {what}')
            if ill:
                # per channel, on the middle block's bn3: its dy comes out of the last block's backward, which is the
                # same launches in both runs, so the two dgammas differ by the summation alone (the first block's dy
                # already carries the difference amplified by the blocks above); the bound of the single-use BN's
                # ill-conditioned-channel test
                tol = {'f32': 1e-4, 'bf16': 2e-2, 'f16': 1e-2}[mode]
                k = names.index('1.bn3.weight')
                a, b = got[k], ref[k]
                top = float(b.abs().max())
                for c in [c for c in range(b.numel()) if c % 4 < 2]:
                    r = float(b[c])
                    assert abs(float(a[c]) - r) <= tol * (abs(r) + 1e-3 * top), (v, c, float(a[c]), r)
                assert float(b[0::4].abs().min()) > 0 and float(b[1::4].abs().min()) > 0   # the true dgamma is not 0
    finally:
        N.call('ssseg_set_knob', 4, 0)
        snn.set_bn_join(True)


def test_bottleneck_stack_join_graph_replay(hip_device):
    """(c) The stack's training pass and its deferred differentiated eval pass captured as one HIP graph: three replays
    are bitwise equal to the same steps issued eagerly (no host read, no allocation outside the caching allocator)."""
    from ssseg import native as N
    from ssseg import nn as snn
    from ssseg.graph import StepGraph
    snn.set_compute_dtype(torch.bfloat16)
    H, W = SHAPES[0]
    gen = torch.Generator().manual_seed(41)
    data = [(snn.to_act(_q(torch.randn(2, 64, H, W, generator=gen), 'bf16').to(hip_device)),
             snn.to_act(_q(torch.randn(2, 64, H, W, generator=gen), 'bf16').to(hip_device))) for _ in range(5)]

    def run(graphed):
        net = _stack(64, 16, hip_device)
        for p in net.parameters():
            p.grad = torch.zeros_like(p)

        def step(x, g):
            outs = []
            for p in net.parameters():
                p.grad.zero_()
            for kind in ('train', 'eval'):
                net.train(kind == 'train')
                xa = x.detach().requires_grad_(True)
                y = net(xa)
                with (snn.defer_param_grads() if kind == 'eval' else contextlib.nullcontext()):
                    y.backward(g)
                outs.append(xa.grad)
            return tuple(outs)

        res = []
        for k in range(2):   # eager steps first: every geometry launched once, the deferred table built
            step(*data[k])
        fn = StepGraph(step, *data[2]) if graphed else step
        for k in range(2, 5):
            out = fn(*data[k])
            torch.cuda.synchronize()
            res.append([t.clone() for t in out] + [p.grad.clone() for p in net.parameters()])
        return res

    N.call('ssseg_set_knob', 5, 0)   # the static variant rule: eager and captured launches pick the same kernels
    try:
        eager = run(False)
        graph = run(True)
    finally:
        N.call('ssseg_set_knob', 5, 1)
    for a, b in zip(eager, graph):
        for s, t in zip(a, b):
            assert torch.isfinite(s.float()).all()
            assert torch.equal(s, t)
