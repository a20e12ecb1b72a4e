"""The conv engine against an fp64 CPU reference under torch.equal, in f32, bf16 and fp16, forward, input gradient and
weight gradient, on every path the engine picks by itself, every forced variant, the fused activations and the fused
backward epilogues.

The operands are small integers (tests/exact.py): every product and every fp32 partial sum is exact in any summation
order and every stored result is representable in the storage dtype (test_conv_exact_host.py proves both for each
case, without a GPU), so the engine must reproduce the reference bit for bit and ONE wrong element anywhere -- a halo
row, a ragged last tile, a border tap, a gradient read from the wrong pixel -- fails the test.  Every comparison is
torch.equal (exact integer equality for padding counts, launch counts and the fp64 statistics); there is no tolerance
in this file.
"""
import contextlib

import pytest
import torch

import exact as E
from test_hip_layers import ALL_VARIANTS

pytestmark = pytest.mark.gpu

KNOBS = (4, 7, 8, 11, 13, 14, 15, 16)


@pytest.fixture(autouse=True)
def _restore_engine_state(hip_device):
    """Knobs, switches and the compute dtype are what the rest of the suite expects, before and after every test."""
    from ssseg import native as N
    from ssseg import nn as snn

    def reset():
        for k in KNOBS:
            N.call('ssseg_set_knob', k, 0)
        snn.set_compute_dtype(torch.bfloat16)
        snn.set_stem_kernel(True)
        snn.set_phase_launch(True)
        snn.set_wgrad_merge(True)
        snn.set_virtual_concat(True)
        snn.set_bn_join(True)
        snn.set_fused_bn_stats(True)
    reset()
    yield
    reset()


@pytest.fixture(params=E.MODES)
def mode(request, _restore_engine_state):
    from ssseg import nn as snn
    snn.set_compute_dtype(E.TORCH_DTYPE[request.param])
    return request.param


@pytest.fixture
def calls(monkeypatch):
    """names of the native launches a test makes (which fused path ran)"""
    from ssseg import native as N
    names = []
    real, real_u = N.call, N.call_or_unsupported

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    def spy_u(name, *a):
        ok = real_u(name, *a)
        if ok:
            names.append(name)
        return ok

    monkeypatch.setattr(N, 'call', spy)
    monkeypatch.setattr(N, 'call_or_unsupported', spy_u)
    return names


def _ids(cases):
    return [c.id for c in cases]


assert_exact = E.assert_exact


@pytest.fixture(scope='module', autouse=True)
def _drop_references():
    """the fp64 references are shared by every mode and variant of this file, and dropped with it"""
    yield
    E.clear_caches()


def assert_zero_padding(t, real, what):
    """the padding channels of a physical activation are zero"""
    if t.shape[1] > real:
        assert int(t.detach()[:, real:].count_nonzero()) == 0, f'{what}: nonzero padding channels'


def _act_arg(act):
    from ssseg import nn as snn
    if act is None:
        return False
    if act == 'relu':
        return True
    return snn.ACT_RELU6 if act == 'relu6' else act


def _dev_act(t, dev, grad=False):
    """fp64 NCHW reference tensor -> the engine's activation (compute dtype, NHWC, padded channels)"""
    from ssseg import nn as snn
    a = snn.to_act(t.float().to(dev)).detach()
    return a.requires_grad_(True) if grad else a


def _module(case, ref, dev, head=False):
    from ssseg import nn as snn
    if case.kind == 'convT':
        m = snn.ConvTranspose2d(case.cin, case.cout, case.k, case.s, case.p, bias=case.bias)
    elif case.kind == 'dw':
        m = snn.Conv2d(case.cin, case.cout, case.k, case.s, case.p, case.d, groups=case.cin, bias=case.bias)
    else:
        m = snn.Conv2d(case.cin, case.cout, case.k, case.s, case.p, case.d, bias=case.bias, head=head)
    with torch.no_grad():
        m.weight.copy_(ref['w'])
        if case.bias:
            m.bias.copy_(ref['bias'])
    return m.to(dev)


def _run(mod, case, ref, dev, act=None, head=False):
    mod.zero_grad(set_to_none=True)
    xa = _dev_act(ref['x'], dev, grad=True)
    y = mod(xa) if act is None else mod.forward_act(xa, _act_arg(act))
    y.backward(ref['gy'].float().to(dev) if head else _dev_act(ref['gy'], dev))
    torch.cuda.synchronize()
    return {'y': y.detach(), 'dx': xa.grad, 'dW': mod.weight.grad, 'db': mod.bias.grad if case.bias else None}


def _check(got, ref, case, mode, what, shift=0, head=False, names=('y', 'dx', 'dW', 'db')):
    fp32 = E.FP32_OUTPUTS + (('y',) if head else ())
    E.check_exact_range(E.outputs(ref, names), mode, shift, fp32)   # the comparison below is legitimate
    real = {'y': case.cout, 'dx': case.cin}
    for name in names:
        if ref.get(name) is None:
            continue
        t = got[name]
        if name in real:
            if not (head and name == 'y'):
                assert_zero_padding(t, real[name], f'{what} {name}')
            t = t[:, :real[name]]
        assert_exact(t, ref[name], f'{what} {name}')


def _case_test(case, mode, dev, act=None, head=False, tag='', variants=(0,)):
    from ssseg import native as N
    for regime in E.REGIMES:
        ref = E.reference(case, regime, act)
        mod = _module(case, ref, dev, head)
        for v in variants:
            N.call('ssseg_set_knob', 4, v)
            _check(_run(mod, case, ref, dev, act, head), ref, case, mode,
                   f'{case.id} {regime} {mode}{tag}' + (f' variant {v}' if v else ''), E.act_shift(act), head)


# ---------------------------------------------------------------------------------------------------------------------
# a. every path the engine picks by itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', E.AUTO_CASES, ids=_ids(E.AUTO_CASES))
def test_conv_auto(hip_device, mode, case):
    """y, dx, dW of the kernels the engine chooses (register-staged, LDS-DMA tile configs, general-k loader, virtual
    pad, halo, pointwise, split-K; the fp32 kernels in f32 mode), random integer gy, both regimes."""
    _case_test(case, mode, hip_device)


@pytest.mark.parametrize('case', E.CONV_CASES, ids=_ids(E.CONV_CASES))
def test_conv_head_auto(hip_device, mode, case):
    """head=True: fp32 logits with the real channel count visible, fp32 NCHW gradient in"""
    _case_test(case, mode, hip_device, head=True)


@pytest.mark.parametrize('stem', [True, False], ids=['stem', 'generic'])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('case', E.STEM, ids=_ids(E.STEM))
def test_conv_stem(hip_device, case, dtype, stem):
    """the image-input kernel (ssseg_conv_stem_epi) and the generic engine on the same 3 -> 64 layers"""
    from ssseg import nn as snn
    snn.set_compute_dtype(E.TORCH_DTYPE[dtype])
    snn.set_stem_kernel(stem)
    _case_test(case, dtype, hip_device, tag=' stem' if stem else ' generic')


@pytest.mark.parametrize('phases', [True, False], ids=['one-launch', 'per-phase'])
@pytest.mark.parametrize('case', E.CONVT, ids=_ids(E.CONVT))
def test_conv_transpose_auto(hip_device, mode, case, phases):
    """ConvTranspose2d(4, 2, 1) with bias: one launch over the four output phases, and one launch per phase"""
    from ssseg import nn as snn
    snn.set_phase_launch(phases)
    _case_test(case, mode, hip_device, tag=' phases' if phases else ' per-phase')


@pytest.mark.parametrize('case', E.DEPTHWISE, ids=_ids(E.DEPTHWISE))
def test_depthwise_auto(hip_device, mode, case):
    _case_test(case, mode, hip_device)


# ---------------------------------------------------------------------------------------------------------------------
# b. every forced variant (bf16), the knobs, the merged two-pass weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('case', E.VARIANT_CASES, ids=_ids(E.VARIANT_CASES))
def test_conv_forced_variants(hip_device, case, regime):
    """ssseg_set_knob(4, v) for every variant: y, dx and dW against the REFERENCE (not against another variant), random
    integer gy.  A variant the engine refuses for a geometry falls back by design."""
    from ssseg import native as N
    ref = E.reference(case, regime)
    mod = _module(case, ref, hip_device)
    for v in ALL_VARIANTS:
        N.call('ssseg_set_knob', 4, v)
        _check(_run(mod, case, ref, hip_device), ref, case, 'bf16', f'{case.id} {regime} variant {v}')


KNOB_PARAMS = [pytest.param(k, v, c, id=f'knob{k}={v}-{c.id}') for k, v, cases in E.KNOB_CASES for c in cases]


@pytest.mark.parametrize('knob,value,case', KNOB_PARAMS)
def test_conv_knobs(hip_device, knob, value, case):
    """register-staged weight gradient (8), halo kernels off (11), pointwise kernels off (13), split-K off / forced
    S (14), LDS-staged epilogue off (7), 64-wide halo tiles only (16): y, dx, dW, both regimes"""
    from ssseg import native as N
    N.call('ssseg_set_knob', knob, value)
    _case_test(case, 'bf16', hip_device, tag=f' knob {knob} = {value}')


STALE_ROWS = E.STALE_ROWS


@pytest.mark.parametrize('knob,variant,case', STALE_ROWS, ids=[f'knob{k}-v{v}-{c.id}' for k, v, c in STALE_ROWS])
def test_cached_variant_of_a_switched_off_family_falls_back(hip_device, knob, variant, case):
    """What test_conv_knobs[knob13=-1, 128 -> 64 1x1 at 17 x 20] caught: the variant table (filled by the autotuner, or
    loaded from a file / another rank by ssseg.tune) named the pointwise kernel for a geometry, knob 13 = -1 then
    switched that family off, and the launch failed with SSSEG_EUNSUPPORTED instead of running another kernel (the same
    for the halo kernels behind knobs 11 / 15, and for an imported row naming a kernel that does not apply).  Here every
    row of the table is pointed at the family's variant, so the case's forward and input-gradient launches find it
    cached: exact results with the family on, and exact results -- not an error -- with it off."""
    from ssseg import native as N
    from ssseg import tune
    _case_test(case, 'bf16', hip_device)          # tunes: the case's geometries are in the table
    tuned = tune.export()
    assert len(tuned) > 0
    try:
        tune.import_([(k, variant) for k, _ in tuned], overwrite=True)
        _case_test(case, 'bf16', hip_device, tag=f' cached variant {variant}')
        N.call('ssseg_set_knob', knob, -1)
        _case_test(case, 'bf16', hip_device, tag=f' cached variant {variant}, knob {knob} = -1')
    finally:
        N.call('ssseg_set_knob', knob, 0)
        tune.import_(tuned, overwrite=True)


@pytest.mark.parametrize('knob,value', [(0, 0), (8, -1), (11, -1)], ids=['default', 'register-staged', 'no-halo'])
@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('case', E.MERGED_CASES, ids=_ids(E.MERGED_CASES))
def test_wgrad_merged_two_passes_exact(hip_device, case, regime, knob, value):
    """defer_wgrad + the next backward + flush_wgrad, batches (2, 3): ONE launch over both pixel sets gives exactly
    the sum of the two passes' weight (and bias) gradients, on both weight-gradient kernels and the halo one."""
    from ssseg import native as N
    from ssseg import nn as snn
    if knob:
        N.call('ssseg_set_knob', knob, value)
    refs = [E.reference(case._replace(n=n), regime) for n in (2, 3)]
    want = {'dW': refs[0]['dW'] + refs[1]['dW'], 'db': refs[0]['db'] + refs[1]['db'] if case.bias else None}
    E.check_exact_range(want, 'bf16')
    mod = _module(case, refs[0], hip_device)
    for i, r in enumerate(refs):
        y = mod(_dev_act(r['x'], hip_device))
        with (snn.defer_wgrad() if i == 0 else contextlib.nullcontext()):
            y.backward(_dev_act(r['gy'], hip_device))
        if i == 0:
            assert snn.wgrad_pending() == 1
    snn.flush_wgrad()
    assert snn.wgrad_pending() == 0
    torch.cuda.synchronize()
    assert_exact(mod.weight.grad, want['dW'], f'{case.id} {regime} merged dW')
    if case.bias:
        assert_exact(mod.bias.grad, want['db'], f'{case.id} {regime} merged db')


# ---------------------------------------------------------------------------------------------------------------------
# c. fused activations in all three modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', E.ACTS, ids=['relu', 'relu6', 'leaky'])
@pytest.mark.parametrize('case', E.ACT_CASES, ids=_ids(E.ACT_CASES))
def test_conv_fused_activation(hip_device, mode, case, act):
    """Conv2d.forward_relu / forward_act(ACT_RELU6) / forward_act(('leaky', 0.25)) with bias: y, dx, dW, db against the
    fp64 reference of the composite.  Integer pre-activations: no output lies within rounding of 0 or 6, so the mask
    has no near-ties in any mode; the slope 2^-2 keeps every value a multiple of 1/4 (shift 2).  bf16: on every engine
    variant."""
    _case_test(E.act_case(case, act), mode, hip_device, act=act, variants=ALL_VARIANTS if mode == 'bf16' else (0,))


@pytest.mark.parametrize('phases', [True, False], ids=['one-launch', 'per-phase'])
@pytest.mark.parametrize('case', E.CONVT[:2], ids=_ids(E.CONVT[:2]))
def test_conv_transpose_fused_relu(hip_device, mode, case, phases):
    from ssseg import nn as snn
    snn.set_phase_launch(phases)
    _case_test(case, mode, hip_device, act='relu')


@pytest.mark.parametrize('case', E.DEPTHWISE, ids=_ids(E.DEPTHWISE))
def test_depthwise_fused_relu6(hip_device, mode, case):
    _case_test(case, mode, hip_device, act='relu6')


# ---------------------------------------------------------------------------------------------------------------------
# d. fused backward epilogues against the fp64 reference of the unfused math
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('act', E.CHAIN_ACTS, ids=['relu', 'leaky'])
def test_producer_activation_mask_exact(hip_device, mode, calls, act, regime):
    """forward_act(..., single_use=True) feeding a second conv: the consumer's input-gradient launch applies the
    producer's activation backward (ssseg_conv_igemm_epi_actmask).  h, y, dx, dW1, db1, dW2 against fp64 autograd of
    the two plain layers."""
    from ssseg import nn as snn
    ref = E.chain_reference(act, regime)
    shift = E.act_shift(act)
    E.check_exact_range({k: ref[k] for k in ('h', 'y', 'dx', 'dW1', 'db1', 'dW2')}, mode, shift)
    c1 = snn.Conv2d(8, 32, 4, 2, 1).to(hip_device)
    c2 = snn.Conv2d(32, 48, 4, 2, 1).to(hip_device)
    with torch.no_grad():
        for p, k in ((c1.weight, 'w1'), (c1.bias, 'b1'), (c2.weight, 'w2'), (c2.bias, 'b2')):
            p.copy_(ref[k])
    xa = _dev_act(ref['x'], hip_device, grad=True)
    h = c1.forward_act(xa, _act_arg(act), single_use=True)
    y = c2(h)
    del calls[:]
    y.backward(_dev_act(ref['gy'], hip_device))
    torch.cuda.synchronize()
    # the consumer's input-gradient launches carry the mask; no separate activation backward
    assert 'ssseg_conv_igemm_epi_actmask' in calls and 'ssseg_act_bwd' not in calls
    what = f'chain {act} {regime} {mode}'
    assert_exact(h[:, :32], ref['h'], what + ' h')
    assert_exact(y[:, :48], ref['y'], what + ' y')
    assert_exact(xa.grad[:, :8], ref['dx'], what + ' dx')
    assert_zero_padding(y, 48, what + ' y')
    assert_exact(c1.weight.grad, ref['dW1'], what + ' dW1')
    assert_exact(c1.bias.grad, ref['db1'], what + ' db1')
    assert_exact(c2.weight.grad, ref['dW2'], what + ' dW2')


@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('cin,cout,H,W', E.JOIN_CASES)
def test_join_dgrad_exact(hip_device, mode, calls, cin, cout, H, W, regime):
    """The residual-join input gradient (ssseg_conv_igemm_epi_join, reached as tests/test_bn_join.py reaches it): a 1x1
    conv's dgrad plus the shortcut gradient, masked by the join's ReLU, equals relu'(z) * (W^T gy + add) exactly -- on
    every engine variant in bf16."""
    from ssseg import native as N
    from ssseg import nn as snn
    ref = E.join_reference(cin, cout, H, W, regime)
    E.check_exact_range({'dx': ref['dx']}, mode)
    conv = snn.Conv2d(cin, cout, 1, bias=False).to(hip_device)
    with torch.no_grad():
        conv.weight.copy_(ref['w'])
    gy, z, add = (_dev_act(ref[k], hip_device) for k in ('gy', 'z', 'add'))
    for v in (ALL_VARIANTS if mode == 'bf16' else [0]):
        N.call('ssseg_set_knob', 4, v)
        del calls[:]
        dx = conv._ssseg_dgrad(gy, z.shape, residual=add, join=z)
        torch.cuda.synchronize()
        assert calls.count('ssseg_conv_igemm_epi_join') == 1, f'variant {v}: the engine declined the join epilogue'
        assert_exact(dx[:, :cin], ref['dx'], f'join {cin}->{cout} {H}x{W} {regime} {mode} variant {v} dx')


@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('ca,cb,H,W', E.VCAT_CASES)
def test_virtual_concat_exact(hip_device, mode, calls, ca, cb, H, W, regime):
    """cat_crop(..., lazy=True) feeding a 3x3 conv: the forward reads the two parts where they lie and the input
    gradient is written straight into the parts' gradients (ssseg_conv_igemm_epi_vsplit) in the 16-bit modes; f32 takes
    the ordinary concat.  y, both part gradients and dW."""
    from ssseg import nn as snn
    ref = E.vcat_reference(ca, cb, H, W, regime)
    E.check_exact_range({k: ref[k] for k in ('y', 'da', 'db_part', 'dW')}, mode, fp32=('dW',))
    conv = snn.Conv2d(ca + cb, 64, 3, 1, 1, bias=False).to(hip_device)
    with torch.no_grad():
        conv.weight.copy_(ref['w'])
    a = _dev_act(ref['a'].contiguous(), hip_device, grad=True)
    b = _dev_act(ref['b'].contiguous(), hip_device, grad=True)
    cat = snn.cat_crop(a, b, ca, cb, lazy=True)
    y = conv(cat)
    y.backward(_dev_act(ref['gy'], hip_device))
    torch.cuda.synchronize()
    virtual = 0 if mode == 'f32' else 1
    assert calls.count('ssseg_conv_igemm_epi_vcat') == virtual and calls.count('ssseg_conv_igemm_epi_vsplit') == virtual
    what = f'vcat {ca}+{cb} {H}x{W} {regime} {mode}'
    assert_exact(y[:, :64], ref['y'], what + ' y')
    assert_exact(a.grad[:, :ca], ref['da'], what + ' da')
    assert_exact(b.grad[:, :cb], ref['db_part'], what + ' db')
    assert_exact(conv.weight.grad, ref['dW'], what + ' dW')


# ---------------------------------------------------------------------------------------------------------------------
# e. folded eval BatchNorm epilogue with residual and ReLU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('case', E.FOLD_CASES, ids=_ids(E.FOLD_CASES))
def test_folded_eval_bn_residual_relu_exact(hip_device, mode, calls, case, regime):
    """conv_bn_act in eval mode with a residual and ReLU (the Bottleneck tail), differentiated: eps = 0, running_var in
    {0.25, 1, 4}, gamma a power of two, integer running_mean / beta / residual make the device fold (scale = gamma /
    sqrt(var), shift = beta - mean * scale) and the epilogue acc * scale + shift + residual exact: y, dx, dres and dW
    equal the fp64 reference (multiples of 1/2: shift 1) -- on every engine variant in bf16."""
    from ssseg import native as N
    from ssseg import nn as snn
    ref = E.fold_reference(case, regime)
    E.check_exact_range({k: ref[k] for k in ('y', 'dx', 'dres', 'dW')}, mode, 1)
    mc = _module(case, ref, hip_device)
    mb = snn.BatchNorm2d(case.cout)
    mb.eps = 0.0
    with torch.no_grad():
        for p, k in ((mb.weight, 'gamma'), (mb.bias, 'beta'), (mb.running_mean, 'mean'), (mb.running_var, 'var')):
            p.copy_(ref[k])
    mb = mb.to(hip_device).eval()
    for v in (ALL_VARIANTS if mode == 'bf16' else [0]):
        N.call('ssseg_set_knob', 4, v)
        mc.zero_grad(set_to_none=True)
        mb.zero_grad(set_to_none=True)
        xa = _dev_act(ref['x'], hip_device, grad=True)
        ra = _dev_act(ref['res'], hip_device, grad=True)
        del calls[:]
        y = snn.conv_bn_act(mc, xa, mb, relu=True, residual=ra)
        y.backward(_dev_act(ref['gy'], hip_device))
        torch.cuda.synchronize()
        assert calls.count('ssseg_bn_apply') == 0   # folded: no separate BatchNorm pass
        what = f'fold {case.id} {regime} {mode} variant {v}'
        assert_exact(y[:, :case.cout], ref['y'], what + ' y')
        assert_zero_padding(y, case.cout, what + ' y')
        assert_exact(ra.grad[:, :case.cout], ref['dres'], what + ' dres')
        assert_exact(xa.grad[:, :case.cin], ref['dx'], what + ' dx')
        assert_zero_padding(xa.grad, case.cin, what + ' dx')
        assert_exact(mc.weight.grad, ref['dW'], what + ' dW')


# ---------------------------------------------------------------------------------------------------------------------
# f. fused BatchNorm statistics: the fp64 partial rows of the conv epilogue
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', E.STATS_CASES, ids=_ids(E.STATS_CASES))
def test_fused_bn_statistics_exact(hip_device, mode, case):
    """The rows a conv's epilogue writes for a training BatchNorm (ssseg_conv_epilogue.stats: per output tile, sum y
    and sum y^2 in fp64 of the value as stored) add up to the exact integer sums of the reference output, per channel --
    on every engine variant in bf16."""
    from ssseg import native as N
    from ssseg import nn as snn
    for regime in E.REGIMES:
        ref = E.reference(case, regime)
        want = E.stats_reference(case, regime)
        E.check_exact_range(want, mode)
        mod = _module(case, ref, hip_device)
        xa = _dev_act(ref['x'], hip_device)
        cap = mod.stat_rows_cap(case.n, case.H, case.W)
        assert cap is not None and cap > 0
        for v in (ALL_VARIANTS if mode == 'bf16' else [0]):
            N.call('ssseg_set_knob', 4, v)
            rows = snn.StatRows(case.cout, cap, hip_device)
            with torch.no_grad():
                y = mod(xa, stats=rows)
            torch.cuda.synchronize()
            what = f'{case.id} {regime} {mode} variant {v}'
            assert 0 < rows.rows <= cap, what
            part = rows.part[:2 * rows.rows * case.cout].view(rows.rows, 2, case.cout).sum(0).cpu()
            assert_exact(part[0], want['sum'], what + ' sum y')
            assert_exact(part[1], want['sumsq'], what + ' sum y^2')
            assert_exact(y[:, :case.cout], ref['y'], what + ' y')
