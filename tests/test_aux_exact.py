"""The kernels between the convolutions -- BatchNorm (csrc/bn.hip), the pools, the n-ary add, dropout and the attention
blend (csrc/pool.hip), max-pool, copies and the activation backward (csrc/misc.hip), concat / split (csrc/cat.hip) and
the NHWC bilinear resize (csrc/interp.hip) -- against an fp64 CPU reference of the plain PyTorch operation, in f32,
bf16 and fp16, forward and backward.

Tier A compares under torch.equal on operands whose every intermediate is exact (tests/exact_aux.py;
test_aux_exact_host.py proves range and non-degeneracy for each case without a GPU), so ONE wrong element -- a dropped
tail pixel, a chunk read from the neighbouring pixel, a dead slot of the unrolled pixel loop that is not skipped, a
nonzero padding channel -- fails the test.  Tier B, where the arithmetic cannot be exact, bounds EVERY element by
1/2 ulp_store(ref) + k 2^-24 M with k counted from the kernel source (exact_aux.py states each).  No comparison is with
another of our kernels, and there is no mean, no relative or absolute tolerance in this file except the stated bound
on running_var (the unbiased factor P / (P - 1) is not dyadic: one fp32 rounding of the kernel's fp64 value plus the
reference's own cast, 2^-22 relative).
"""
import pytest
import torch

import exact as E
import exact_aux as A

pytestmark = pytest.mark.gpu

assert_exact = E.assert_exact


@pytest.fixture(params=E.MODES)
def mode(request, hip_device):
    from ssseg import nn as snn
    snn.set_compute_dtype(E.TORCH_DTYPE[request.param])
    yield request.param
    snn.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope='module', autouse=True)
def _drop_references():
    yield
    A.clear_caches()


def _dev(t, dev, grad=False):
    """fp64 NCHW reference tensor -> the engine's activation (compute dtype, NHWC, zero-padded channels)"""
    from ssseg import nn as snn
    if t is None:
        return None
    a = snn.to_act(t.float().to(dev)).detach()
    return a.requires_grad_(True) if grad else a


def _same(got, want, what):
    """an activation against its NCHW reference: the real channels equal, the padding channels zero"""
    C = want.shape[1]
    assert_exact(got.detach()[:, :C], want, what)
    if got.shape[1] > C:
        assert int(got.detach()[:, C:].count_nonzero()) == 0, f'{what}: nonzero padding channels'


def _act_arg(act):
    return False if act is None else True if act == 'relu' else act


def _f32(t, dev):
    return t.float().to(dev).contiguous()


def _rows(t, ld, dev, dtype, fill=0.0):
    """fp64 NCHW -> a [P, ld] device matrix of `dtype` (NHWC with leading dimension ld), padding = fill"""
    n, c, h, w = t.shape
    m = torch.full((n * h * w, ld), fill, dtype=torch.float64)
    m[:, :c] = t.permute(0, 2, 3, 1).reshape(-1, c)
    return m.to(dtype).to(dev).contiguous()


def _unrows(m, like):
    n, c, h, w = like.shape
    return m.detach().cpu()[:, :c].reshape(n, h, w, c).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
def _bn_module(C, gamma, beta, rmean, rvar, dev, train):
    from ssseg import nn as snn
    bn = snn.BatchNorm2d(C, momentum=A.BN_MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rmean)
        bn.running_var.copy_(rvar)
    bn.eps = 0.0
    bn = bn.to(dev)
    return bn.train() if train else bn.eval()


def _bn_run(bn, ref, dev, relu, residual):
    from ssseg import nn as snn
    xa, ra = _dev(ref['x'], dev, grad=True), _dev(ref['res'], dev, grad=True) if residual else None
    y = snn.bn_act(xa, bn, relu=relu, residual=ra)
    y.backward(_dev(ref['gy'], dev))
    torch.cuda.synchronize()
    return {'y': y, 'dx': xa.grad, 'dres': ra.grad if residual else None, 'dgamma': bn.weight.grad,
            'dbeta': bn.bias.grad}


@pytest.mark.parametrize('relu,residual', A.BN_FLAGS)
@pytest.mark.parametrize('C,nhw', A.BN_CASES, ids=[A.bn_id(*c) for c in A.BN_CASES])
def test_bn_train_exact(hip_device, mode, C, nhw, relu, residual):
    """Train-mode bn_act with designed statistics (mean = m, invstd = 1 / s, x_hat = r exactly): y, dx, dres, dgamma,
    dbeta and running_mean equal the fp64 reference, the padding channels are zero, running_var holds to 2^-22."""
    C = A.chans(C, mode)
    ref = A.bn_train_reference(C, nhw, relu, residual)
    A.bn_train_check_range(ref, mode)
    bn = _bn_module(C, ref['gamma'], ref['beta'], ref['rm0'], ref['rv0'], hip_device, True)
    got = _bn_run(bn, ref, hip_device, relu, residual)
    for name in ('y', 'dx') + (('dres',) if residual else ()):
        _same(got[name], ref[name], name)
    assert_exact(got['dgamma'], ref['dgamma'], 'dgamma')
    assert_exact(got['dbeta'], ref['dbeta'], 'dbeta')
    assert_exact(bn.running_mean, ref['running_mean'], 'running_mean')
    rv = bn.running_var.detach().double().cpu()
    assert bool(((rv - ref['running_var']).abs() <= 2.0 ** -22 * ref['running_var'].abs()).all()), 'running_var'


@pytest.mark.parametrize('relu,residual', A.BN_FLAGS)
def test_bn_train_exact_8_byte_chunks(hip_device, mode, relu, residual):
    """The native ABI on buffers whose leading dimension is 4 mod 8 (C = 10, ld = 12: HarDNet's widths), where the
    16-bit kernels fall back to 8-byte chunks; to_act cannot produce such a buffer.  Outputs are prefilled with 7: the
    padding channels [C, 12) must come back 0."""
    from ssseg import native as N
    C, ld, nhw = 10, 12, A.BN_MAP
    ref = A.bn_train_reference(C, nhw, relu, residual)
    A.bn_train_check_range(ref, mode)
    dev, dt = hip_device, E.TORCH_DTYPE[mode]
    P = nhw[0] * nhw[1] * nhw[2]
    x, gy = _rows(ref['x'], ld, dev, dt), _rows(ref['gy'], ld, dev, dt)
    res = _rows(ref['res'], ld, dev, dt) if residual else None
    y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    dres = torch.full_like(x, 7.0) if residual else None
    gamma, beta = _f32(ref['gamma'], dev), _f32(ref['beta'], dev)
    rm, rv = _f32(ref['rm0'], dev), _f32(ref['rv0'], dev)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    dgamma, dbeta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
    nb = N.lib().ssseg_bn_workspace_bytes(C)
    ws = N.workspace(nb, dev)
    code, p, s = int(relu), N.dev_ptr, N.stream()
    N.call('ssseg_bn_stats_finalize', p(x), P, C, ld, N.dt_code(x), p(sums), p(ws), nb, float(P), 0.0, A.BN_MOMENTUM,
           p(mean), p(invstd), p(rm), p(rv), None, s)
    N.call('ssseg_bn_apply', p(x), p(res), p(y), P, C, ld, ld, ld, p(mean), p(invstd), p(gamma), p(beta), code,
           N.dt_code(x), s)
    N.call('ssseg_bn_bwd_reduce_grad', p(gy), p(x), p(res), P, C, ld, ld, ld, p(mean), p(invstd), p(gamma), p(beta),
           code, N.dt_code(x), p(sums), p(ws), nb, p(dgamma), p(dbeta), s)
    N.call('ssseg_bn_bwd_apply', p(gy), p(x), p(res), p(dx), p(dres), P, C, ld, ld, ld, ld, p(mean), p(invstd),
           p(gamma), p(beta), code, 1, p(sums), float(P), N.dt_code(x), s)
    torch.cuda.synchronize()
    assert_exact(mean, ref['mean'], 'mean')
    assert_exact(invstd, ref['invstd'], 'invstd')
    for name, m in (('y', y), ('dx', dx)) + ((('dres', dres),) if residual else ()):
        assert_exact(_unrows(m, ref[name]), ref[name], name)
        assert int(m[:, C:].count_nonzero()) == 0, f'{name}: padding channels not written as zero'
    assert_exact(dgamma, ref['dgamma'], 'dgamma')
    assert_exact(dbeta, ref['dbeta'], 'dbeta')
    assert_exact(rm, ref['running_mean'], 'running_mean')


@pytest.mark.parametrize('relu,residual', A.BN_FLAGS)
@pytest.mark.parametrize('C,nhw', A.BN_EVAL_CASES, ids=[A.bn_id(*c) for c in A.BN_EVAL_CASES])
def test_bn_eval_exact(hip_device, mode, C, nhw, relu, residual):
    """Eval-mode bn_act with an exactly representable fold: forward, dx, dres, dgamma, dbeta."""
    C = A.chans(C, mode)
    ref = A.bn_eval_reference(C, nhw, relu, residual)
    A.bn_eval_check_range(ref, mode)
    bn = _bn_module(C, ref['gamma'], ref['beta'], ref['mean'], ref['var'], hip_device, False)
    got = _bn_run(bn, ref, hip_device, relu, residual)
    for name in ('y', 'dx') + (('dres',) if residual else ()):
        _same(got[name], ref[name], name)
    assert_exact(got['dgamma'], ref['dgamma'], 'dgamma')
    assert_exact(got['dbeta'], ref['dbeta'], 'dbeta')
    assert_exact(bn.running_mean, ref['mean'], 'running_mean (eval: untouched)')


# (the from-y path exists only without a residual)
EVAL_BWD_PATHS = [(False, relu, res) for relu, res in A.BN_FLAGS] + [(True, False, False), (True, True, False)]


@pytest.mark.parametrize('from_y,relu,residual', EVAL_BWD_PATHS,
                         ids=[f'{"from-y" if f else "aux"}-relu{int(r)}-res{int(s)}' for f, r, s in EVAL_BWD_PATHS])
@pytest.mark.parametrize('C,nhw', A.BN_EVAL_CASES, ids=[A.bn_id(*c) for c in A.BN_EVAL_CASES])
def test_bn_eval_bwd_entry_points_exact(hip_device, mode, C, nhw, relu, residual, from_y):
    """ssseg_bn_fold and the folded-BN backward (ssseg_bn_eval_bwd_grad from the raw accumulator copy,
    ssseg_bn_eval_bwd_grad_y from the stored output where there is no residual): dconv = scale dyr, dres = dyr,
    dgamma, dbeta and the conv bias gradient scale * sum dyr."""
    from ssseg import native as N
    C = A.chans(C, mode)
    ref = A.bn_eval_reference(C, nhw, relu, residual)
    A.bn_eval_check_range(ref, mode)
    dev, p, s = hip_device, N.dev_ptr, N.stream()
    P = nhw[0] * nhw[1] * nhw[2]
    scale, shift, mean_eff, invstd = (torch.empty(C, device=dev) for _ in range(4))
    rmean, rvar, gamma, beta = (_f32(ref[k], dev) for k in ('mean', 'var', 'gamma', 'beta'))   # (kept alive)
    N.call('ssseg_bn_fold', p(rmean), p(rvar), p(gamma), p(beta), None, 0.0, C, C, p(scale), p(shift), p(mean_eff),
           p(invstd), s)
    for name, t in (('scale', scale), ('shift', shift), ('mean', mean_eff), ('invstd', invstd)):
        assert_exact(t, ref[name], f'fold {name}')
    aux, ya, gy = _dev(ref['x'], dev), _dev(ref['y'], dev), _dev(ref['gy'], dev)
    ld = aux.shape[1]
    dconv = torch.full_like(aux, 7.0)
    dres = torch.full_like(aux, 7.0) if residual else None
    dgamma, dbeta, dbias = (torch.zeros(C, device=dev) for _ in range(3))
    sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
    nb = N.lib().ssseg_bn_workspace_bytes(C)
    ws = N.workspace(nb, dev)
    if from_y:
        N.call('ssseg_bn_eval_bwd_grad_y', p(gy), p(ya), p(dconv), p(dres), P, C, ld, p(scale), p(shift), p(mean_eff),
               p(invstd), int(relu), N.dt_code(gy), p(sums), p(ws), nb, p(dgamma), p(dbeta), p(dbias), s)
    else:
        N.call('ssseg_bn_eval_bwd_grad', p(gy), p(ya), p(aux), p(dconv), p(dres), P, C, ld, p(scale), p(mean_eff),
               p(invstd), int(relu), N.dt_code(gy), p(sums), p(ws), nb, p(dgamma), p(dbeta), p(dbias), s)
    torch.cuda.synchronize()
    _same(dconv, ref['dx'], 'dconv')
    if residual:
        _same(dres, ref['dres'], 'dres')
    assert_exact(dbeta, ref['dbeta'], 'dbeta')
    assert_exact(dbias, ref['dbeta'] * ref['scale'], 'dconv_bias')
    # (from y, x_hat is recoverable only where a ReLU leaves dyr != 0: exactly where it counts)
    assert_exact(dgamma, ref['dgamma'], 'dgamma')


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: pools
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op,C,hw', [pytest.param(*c, id=A.pool_id(*c)) for c in A.POOL_CASES])
def test_pool_exact(hip_device, mode, op, C, hw):
    """MaxPool2d 3/2/1 and 2/2/0-ceil on tie-heavy integers (the gradient goes to the FIRST maximum), AvgPool2d 2/2/0;
    the avg-pool gradient of the odd row / column no window reaches is zero (part of dx)."""
    from ssseg import nn as snn
    kind, k, s, p, ceil = op
    ref = A.pool_reference(op, C, hw)
    E.check_exact_range({n: ref[n] for n in ('y', 'dx')}, mode, 2 if kind == 'avg' else 0)
    mod = snn.MaxPool2d(k, s, p, ceil_mode=ceil) if kind == 'max' else snn.AvgPool2d(k, s, p)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = mod(xa)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    _same(xa.grad, ref['dx'], 'dx')


@pytest.mark.parametrize('op,C,hw', [pytest.param(*c, id=A.pool_id(*c)) for c in A.POOL_CASES if c[0][0] == 'max'])
def test_maxpool_bwd_res_exact(hip_device, mode, op, C, hw):
    """ssseg_maxpool_bwd_res: the gathered gradient plus a parked gradient of x, in one pass"""
    from ssseg import native as N
    _, k, s, p, _ = op
    ref = A.pool_reference(op, C, hw)
    E.check_exact_range({'dx_add': ref['dx_add']}, mode)
    dev, ptr = hip_device, N.dev_ptr
    xa, gy, add = _dev(ref['x'], dev), _dev(ref['gy'], dev), _dev(ref['add'], dev)
    n, c, h, w = xa.shape
    oh, ow = ref['y'].shape[2:]
    y = torch.empty((n, c, oh, ow), dtype=xa.dtype, device=dev, memory_format=torch.channels_last)
    idx = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=dev)
    gx = torch.full_like(xa, 7.0)
    N.call('ssseg_maxpool_fwd', ptr(xa), ptr(y), ptr(idx), n, h, w, c, oh, ow, k, s, p, N.dt_code(xa), N.stream())
    N.call('ssseg_maxpool_bwd_res', ptr(gy), ptr(idx), ptr(add), ptr(gx), n, h, w, c, oh, ow, k, s, p, N.dt_code(xa),
           N.stream())
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    _same(gx, ref['dx_add'], 'dx + add')


@pytest.mark.parametrize('C,H,W', A.GAP_CASES)
def test_global_avgpool_exact(hip_device, mode, C, H, W):
    """HW = 64 (one split), 1024 (four splits), C = 520 (the second block of 64 channel chunks in the 16-bit modes)"""
    from ssseg import nn as snn
    C = A.chans(C, mode)
    ref = A.gap_reference(C, H, W)
    E.check_exact_range({n: ref[n] for n in ('y', 'dx')}, mode, (H * W).bit_length() - 1)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = snn.global_avgpool(xa)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    _same(xa.grad, ref['dx'], 'dx')


def test_global_avgpool_wide_output_exact(hip_device, mode):
    """ldy > C: the result written into a channel slice of a wider buffer (ASPP's concat), the rest untouched"""
    from ssseg import native as N
    C, H, W = A.chans(A.GAP_CASES[0][0], mode), *A.GAP_CASES[0][1:]
    ref = A.gap_reference(C, H, W)
    dev = hip_device
    xa = _dev(ref['x'], dev)
    n, ldy = xa.shape[0], C + 16
    y = torch.full((n, ldy), 7.0, dtype=xa.dtype, device=dev)
    nb = N.lib().ssseg_global_avgpool_workspace_bytes(n, H * W, C)
    ws = N.workspace(nb, dev)
    N.call('ssseg_global_avgpool_fwd', N.dev_ptr(xa), N.dev_ptr(y), n, H * W, C, ldy, N.dt_code(xa), N.dev_ptr(ws), nb,
           N.stream())
    torch.cuda.synchronize()
    assert_exact(y[:, :C], ref['y'][:, :, 0, 0], 'y')
    assert bool((y[:, C:] == 7.0).all()), 'wrote outside its channel slice'


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: n-ary add, concat, crop, copies, activation backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', A.ADD_ACTS, ids=str)
@pytest.mark.parametrize('n', A.ADD_N)
def test_add_act_exact(hip_device, mode, n, act):
    from ssseg import nn as snn
    ref = A.add_reference(n, act)
    E.check_exact_range({k: ref[k] for k in ('y', 'dx')}, mode, E.act_shift(act))
    xs = [_dev(t, hip_device, grad=True) for t in ref['xs']]
    y = snn.add_act(xs, _act_arg(act))
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    for i, t in enumerate(xs):
        _same(t.grad, ref['dx'], f'dx{i}')


@pytest.mark.parametrize('widths', A.CAT_WIDTHS, ids=str)
def test_cat_n_split_n_exact(hip_device, mode, widths):
    """cat_n / split_n at HarDNet's ragged widths: real channels packed densely, every padding channel zero"""
    from ssseg import nn as snn
    ref = A.cat_reference(widths)
    xs = [_dev(t, hip_device, grad=True) for t in ref['xs']]
    y = snn.cat_n(xs, list(widths))
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    for i, (t, want) in enumerate(zip(xs, ref['dxs'])):
        _same(t.grad, want, f'dx{i}')


@pytest.mark.parametrize('ca,cb,hwa,hwb', A.CROP_CASES)
def test_cat_crop_exact(hip_device, mode, ca, cb, hwa, hwb):
    from ssseg import nn as snn
    ref = A.crop_reference(ca, cb, hwa, hwb)
    a, b = _dev(ref['a'], hip_device, grad=True), _dev(ref['b'], hip_device, grad=True)
    y = snn.cat_crop(a, b, ca, cb)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    _same(a.grad, ref['da'], 'da')
    _same(b.grad, ref['db'], 'db')


@pytest.mark.parametrize('C,sld,dld,c0', [(16, 24, 32, 8), (10, 12, 20, 3)], ids=['v16', 'scalar'])
def test_nhwc_copy_exact(hip_device, mode, C, sld, dld, c0):
    """ssseg_nhwc_copy of a window of a strided source into a channel slice of a wider destination: the 16-byte
    kernel (C, both leading dimensions and the pointers aligned) and the scalar one; nothing else is written."""
    from ssseg import native as N
    dev, dt = hip_device, E.TORCH_DTYPE[mode]
    g = E._gen('copy', C, sld, dld)
    n, sH, sW, dH, dW, H, W, soy, sox, doy, dox = 2, 7, 9, 6, 8, 5, 6, 1, 2, 1, 1
    src = E.ints((n, sH, sW, sld), -3, 3, 1.0, g)
    want = torch.full((n, dH, dW, dld), 9.0, dtype=torch.float64)
    want[:, doy:doy + H, dox:dox + W, c0:c0 + C] = src[:, soy:soy + H, sox:sox + W, :C]
    s = src.to(dt).to(dev)
    d = torch.full((n, dH, dW, dld), 9.0, dtype=dt, device=dev)
    N.call('ssseg_nhwc_copy', N.dev_ptr(s), N.dev_ptr(d) + c0 * d.element_size(), n, H, W, C, sH, sW, sld, soy, sox,
           dH, dW, dld, doy, dox, N.dt_code(s), N.stream())
    torch.cuda.synchronize()
    assert_exact(d, want, 'dst')


@pytest.mark.parametrize('act', A.ACT_BWD, ids=str)
def test_act_bwd_exact(hip_device, mode, act):
    """ssseg_act_bwd / ssseg_relu_bwd with integers ON the boundary points 0 and 6 (strict masks)"""
    from ssseg import native as N
    from ssseg import nn as snn
    ref = A.act_bwd_reference(act)
    E.check_exact_range({'gx': ref['gx']}, mode, E.act_shift(act))
    dev, dt = hip_device, E.TORCH_DTYPE[mode]
    y, gy = ref['y'].to(dt).to(dev), ref['gy'].to(dt).to(dev)
    code, slope = snn._act(_act_arg(act) if act != 'relu6' else snn.ACT_RELU6)
    gx = torch.full_like(gy, 7.0)
    N.call('ssseg_act_bwd', N.dev_ptr(gy), N.dev_ptr(y), N.dev_ptr(gx), gy.numel(), code, slope, N.dt_code(gy),
           N.stream())
    torch.cuda.synchronize()
    assert_exact(gx, ref['gx'], 'gx')
    if act == 'relu':
        gx2 = torch.full_like(gy, 7.0)
        N.call('ssseg_relu_bwd', N.dev_ptr(gy), N.dev_ptr(y), N.dev_ptr(gx2), gy.numel(), N.dt_code(gy), N.stream())
        torch.cuda.synchronize()
        assert_exact(gx2, ref['gx'], 'gx (relu_bwd)')


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: bilinear resize, dropout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,hw,size,ac', [pytest.param(*c, id=A.resize_id(*c)) for c in A.RESIZE_CASES])
def test_resize_act_exact(hip_device, mode, C, hw, size, ac):
    """resize_act where in / out is a power of two: source coordinates and weights are multiples of 1/8 per axis, so
    the forward and the two-pass backward (_bilinear_bwd) are exact multiples of 1/64"""
    from ssseg import nn as snn
    ref = A.resize_reference(C, hw, size, ac)
    E.check_exact_range({k: ref[k] for k in ('y', 'dx')}, mode, A.RESIZE_SHIFT)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = snn.resize_act(xa, size, ac)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _same(y, ref['y'], 'y')
    _same(xa.grad, ref['dx'], 'dx')


@pytest.mark.parametrize('p', A.DROPOUT_P)
def test_dropout_exact(hip_device, mode, p):
    """With integer x every output is 0 or x / (1 - p) exactly, the kept share is 1 - p within 5 sigma of the binomial,
    and the gradient uses the same mask."""
    from ssseg import nn as snn
    x, gy = A.dropout_operands()
    scale = 1.0 / (1.0 - p)
    E.check_exact_range({'x scale': x * scale, 'gy scale': gy * scale}, mode)
    xa = _dev(x, hip_device, grad=True)
    y = snn.Dropout(p).train()(xa)
    y.backward(_dev(gy, hip_device))
    torch.cuda.synchronize()
    yv, gv = y.detach().double().cpu(), xa.grad.double().cpu()
    kept = yv != 0
    zero = torch.zeros_like(x)
    assert torch.equal(yv, torch.where(kept, x * scale, zero)), 'an output that is neither 0 nor x / (1 - p)'
    assert torch.equal(gv, torch.where(kept, gy * scale, zero)), 'the gradient uses another mask'
    n = x.numel()
    assert abs(int(kept.sum()) - n * (1 - p)) <= 5 * (n * p * (1 - p)) ** 0.5, 'kept share'


# ---------------------------------------------------------------------------------------------------------------------
# Tier B: every element within 1/2 ulp_store(ref) + k 2^-24 M
# ---------------------------------------------------------------------------------------------------------------------
def _bounded(got, ref, M, k, mode, what, fp32=False):
    C = ref.shape[1] if ref.dim() == 4 else None
    g = got.detach()
    if C is not None and g.shape[1] > C:
        assert int(g[:, C:].count_nonzero()) == 0, f'{what}: nonzero padding channels'
        g = g[:, :C]
    A.assert_bounded(g, ref, M, k, mode, what, fp32)


@pytest.mark.parametrize('relu,residual', A.BN_FLAGS)
@pytest.mark.parametrize('C,nhw', A.BN_CASES, ids=[A.bn_id(*c) for c in A.BN_CASES])
def test_bn_train_random_bounded(hip_device, mode, C, nhw, relu, residual):
    """Train-mode bn_act on randn data with eps 1e-5 at the Tier A shapes (k = 14 forward, 19 backward, 9 for the
    parameter gradients: exact_aux.py); the residual gradient is a masked copy and must be exact."""
    C = A.chans(C, mode)
    ref = A.bn_train_random(C, nhw, relu, residual, mode)
    bn = _bn_module(C, ref['gamma'], ref['beta'], torch.zeros(C), torch.ones(C), hip_device, True)
    bn.eps = A.BN_EPS
    got = _bn_run(bn, ref, hip_device, relu, residual)
    _bounded(got['y'], ref['y'], ref['My'], A.BN_K_FWD, mode, 'y')
    _bounded(got['dx'], ref['dx'], ref['Mdx'], A.BN_K_BWD, mode, 'dx')
    if residual:
        _bounded(got['dres'], ref['dres'], torch.zeros_like(ref['dres']), 0, mode, 'dres')
    _bounded(got['dgamma'], ref['dgamma'], ref['Mdgamma'], A.BN_K_PGRAD, mode, 'dgamma', fp32=True)
    _bounded(got['dbeta'], ref['dbeta'], ref['Mdbeta'], A.BN_K_PGRAD, mode, 'dbeta', fp32=True)
    A.bn_train_random.cache_clear()


@pytest.mark.parametrize('C,hw', A.AVGPOOL3_CASES)
def test_avgpool3_bounded(hip_device, mode, C, hw):
    """AvgPool2d(3, 2, 1): the divisor 9 is not dyadic (k = 10 forward, 8 backward)"""
    from ssseg import nn as snn
    ref = A.avgpool3_random(C, tuple(hw), mode)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = snn.AvgPool2d(3, 2, 1)(xa)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _bounded(y, ref['y'], ref['My'], A.AVG3_K_FWD, mode, 'y')
    _bounded(xa.grad, ref['dx'], ref['Mdx'], A.AVG3_K_BWD, mode, 'dx')


@pytest.mark.parametrize('C,H,W', A.GAP_RANDOM)
def test_global_avgpool_bounded(hip_device, mode, C, H, W):
    """HW = 143 and 300: 1 / HW is rounded (k = HW + 2 forward, 2 backward)"""
    from ssseg import nn as snn
    ref = A.gap_random(C, H, W, mode)
    kf, kb = A.gap_k(H * W)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = snn.global_avgpool(xa)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _bounded(y, ref['y'], ref['My'], kf, mode, 'y')
    _bounded(xa.grad, ref['dx'], ref['Mdx'], kb, mode, 'dx')


@pytest.mark.parametrize('C,hw,size,ac', [pytest.param(*c, id=A.resize_id(*c)) for c in A.RESIZE_RANDOM])
def test_resize_act_bounded(hip_device, mode, C, hw, size, ac):
    """resize_act at a general size, both align_corners settings (k from exact_aux.resize_k)"""
    from ssseg import nn as snn
    ref = A.resize_random(C, tuple(hw), tuple(size), ac, mode)
    kf, kb = A.resize_k(hw, size)
    xa = _dev(ref['x'], hip_device, grad=True)
    y = snn.resize_act(xa, size, ac)
    y.backward(_dev(ref['gy'], hip_device))
    torch.cuda.synchronize()
    _bounded(y, ref['y'], ref['My'], kf, mode, 'y')
    _bounded(xa.grad, ref['dx'], ref['Mdx'], kb, mode, 'dx')


def test_att_blend_bounded(hip_device):
    """ops.att_blend (fp32 in every compute mode): k = 8 forward, 6 for glo / ghi, 4 C + 12 for the attention
    gradient"""
    from ssseg import ops
    ref = A.att_blend_random()
    lo, hi, att = (ref[k].float().to(hip_device).requires_grad_(True) for k in ('lo', 'hi', 'att'))
    y = ops.att_blend(lo, hi, att)
    y.backward(ref['gy'].float().to(hip_device))
    torch.cuda.synchronize()
    A.assert_bounded(y, ref['y'], ref['My'], A.ATT_K_FWD, 'f32', 'y')
    A.assert_bounded(lo.grad, ref['dlo'], ref['Mg'], A.ATT_K_G, 'f32', 'dlo')
    A.assert_bounded(hi.grad, ref['dhi'], ref['Mg'], A.ATT_K_G, 'f32', 'dhi')
    A.assert_bounded(att.grad, ref['datt'], ref['Matt'], A.att_k_gatt(A.ATT_SHAPE[1]), 'f32', 'datt')
