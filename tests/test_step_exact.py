"""The plumbing kernels every training step passes through -- the NCHW <-> NHWC / dtype converters, the fused clip + SGD
step, the squared norm, the teacher EMA, the loss-scale machinery, axpby / scale / sigmoid (csrc/eltwise.hip) and the
pixel mix (ssseg_mix, csrc/cowmix.hip) -- against the host restatements of tests/exact_step.py.

Every comparison is one of two kinds.  Bit equality (exact_step.same_bits / same_bits_nan, over ALL elements) against a
restatement that test_step_exact_host.py proves on the host: the converters against torch's CPU casts, the SGD step,
the EMA, the loss-scale update, axpby and the scales against numpy float32 with an exact fmaf.  Or a per-element bound
1/2 ulp_store(ref) + k 2^-24 M with k counted from the kernel's expression in the docstring of the exact_step check
(sigmoid, the soft mix, the squared norm of random data, the clip coefficient).  No mean, no tolerance chosen by eye,
no element left out.  The sizes are the smallest at which each path exists: one element, a partial workgroup, the
float4 tail of the EMA, both layout kernels, and one size past each launch's grid cap (the second sweep)."""
import numpy as np
import pytest
import torch

import exact as E
import exact_step as S

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _N():
    from ssseg import native as N
    return N


def _ops():
    from ssseg import ops
    return ops


def _dt(name):
    return E.TORCH_DTYPE[name]


def _np(t):
    return t.detach().cpu().numpy()


def _u16(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# layout and dtype
# ---------------------------------------------------------------------------------------------------------------------
def _convert(entry, src, dst, dims, ld, di, do):
    N = _N()
    N.call(entry, src.data_ptr(), dst.data_ptr(), *dims, ld, S.DT_CODE[di], S.DT_CODE[do], N.stream())
    torch.cuda.synchronize()


def _to_nhwc(x, Cp, di, do, dev):
    """x [N, C, H, W] (CPU, dtype di) through ssseg_nchw_to_nhwc into a NaN-filled [N, H, W, Cp] of dtype do"""
    n, c, h, w = x.shape
    y = torch.full((n, h, w, Cp), NAN, dtype=_dt(do), device=dev)
    _convert('ssseg_nchw_to_nhwc', x.to(dev), y, (n, c, h, w), Cp, di, do)
    return y.cpu()


def _to_nchw(x, C, di, do, dev):
    """x [N, H, W, ldc] (CPU, dtype di) through ssseg_nhwc_to_nchw into a NaN-filled [N, C, H, W] of dtype do"""
    n, h, w, ldc = x.shape
    y = torch.full((n, C, h, w), NAN, dtype=_dt(do), device=dev)
    _convert('ssseg_nhwc_to_nchw', x.to(dev), y, (n, C, h, w), ldc, di, do)
    return y.cpu()


@pytest.mark.parametrize('di,do', S.TO_NHWC_PAIRS, ids=['-'.join(p) for p in S.TO_NHWC_PAIRS])
def test_nchw_to_nhwc(hip_device, di, do):
    """Both kernels (the f32-source pairs take the pixel kernel at Cp % 8 == 0, every other case the generic one), every
    dtype pair, the specials in every case: the bits of permute + torch's CPU cast, +0.0 in the padded lanes of a
    destination that held NaN."""
    n, h, w = S.LAYOUT_NHW
    for C, Cp in S.GENERIC_CCP + S.PIXEL_CCP:
        x = S.values((n, C, h, w), di)
        S.same_bits_nan(_to_nhwc(x, Cp, di, do, hip_device), S.to_nhwc_ref(x, Cp, do), f'{di}->{do} C{C} Cp{Cp}')


@pytest.mark.parametrize('C,Cp', [(3, 8), (3, 4)], ids=['pixel', 'generic'])
def test_nchw_to_nhwc_into_a_slice(hip_device, C, Cp):
    """to_act_cat's call: the second operand's two images land behind the first's three in one buffer of six; the
    bytes before and after the slice stay as they were."""
    N = _N()
    n, h, w = S.LAYOUT_NHW
    x = S.values((n, C, h, w), 'f32')
    buf = torch.full((6, h, w, Cp), 7.0, dtype=torch.bfloat16, device=hip_device)
    off = 3 * h * w * Cp * buf.element_size()
    xd = x.to(hip_device)
    N.call('ssseg_nchw_to_nhwc', xd.data_ptr(), buf.data_ptr() + off, n, C, h, w, Cp, S.DT_CODE['f32'],
           S.DT_CODE['bf16'], N.stream())
    torch.cuda.synchronize()
    want = torch.full((6, h, w, Cp), 7.0, dtype=torch.bfloat16)
    want[3:5] = S.to_nhwc_ref(x, Cp, 'bf16')
    S.same_bits_nan(buf.cpu(), want, f'slice C{C} Cp{Cp}')


@pytest.mark.parametrize('dims,kernel', [(S.BIG_PIXEL, 'pixel'), (S.BIG_GENERIC, 'generic')], ids=['pixel', 'generic'])
def test_nchw_to_nhwc_second_sweep(hip_device, dims, kernel):
    n, C, h, w, Cp = dims
    assert (n * h * w if kernel == 'pixel' else n * h * w * Cp) > S.SWEEP_DEFAULT
    assert (Cp % 8 == 0) == (kernel == 'pixel')
    x = S.values((n, C, h, w), 'f32')
    S.same_bits_nan(_to_nhwc(x, Cp, 'f32', 'bf16', hip_device), S.to_nhwc_ref(x, Cp, 'bf16'), f'second sweep {kernel}')


@pytest.mark.parametrize('di,do', S.TO_NCHW_PAIRS, ids=['-'.join(p) for p in S.TO_NCHW_PAIRS])
def test_nhwc_to_nchw(hip_device, di, do):
    """ldc = Cp for the shapes of the forward converter, and the heads' 2-channel view of an 8-channel buffer; the
    specials sit in the lanes c < C, which the kernel reads"""
    n, h, w = S.LAYOUT_NHW
    for C, ldc in S.GENERIC_CCP + S.PIXEL_CCP + (S.HEAD_VIEW,):
        x = S.values((n, h, w, ldc), di, 'nhwc', lanes=C)
        S.same_bits_nan(_to_nchw(x, C, di, do, hip_device), S.to_nchw_ref(x, C, do), f'{di}->{do} C{C} ldc{ldc}')


def test_nhwc_to_nchw_second_sweep(hip_device):
    n, C, h, w, ldc = S.BIG_NCHW
    assert n * C * h * w > S.SWEEP_DEFAULT
    x = S.values((n, h, w, ldc), 'bf16', 'nhwc', lanes=C)
    S.same_bits_nan(_to_nchw(x, C, 'bf16', 'f32', hip_device), S.to_nchw_ref(x, C, 'f32'), 'second sweep')


def _cast(x, di, do, dev):
    N = _N()
    y = torch.full(x.shape, NAN, dtype=_dt(do), device=dev)
    xd = x.to(dev)
    N.call('ssseg_cast', xd.data_ptr(), y.data_ptr(), x.numel(), S.DT_CODE[di], S.DT_CODE[do], N.stream())
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize('di,do', S.CAST_PAIRS, ids=['-'.join(p) for p in S.CAST_PAIRS])
def test_cast(hip_device, di, do):
    """n = 1 (once per special, and one random value), a partial workgroup, the second sweep"""
    for v in torch.cat([S.SPECIAL_VALUES, torch.tensor([0.7133594], dtype=torch.float32)]):
        x = v.reshape(1).to(_dt(di))
        S.same_bits_nan(_cast(x, di, do, hip_device), S.cast_ref(x, do), f'{di}->{do} n=1 v={float(v)!r}')
    for n in S.CAST_N[1:]:
        x = S.values((n,), di)
        S.same_bits_nan(_cast(x, di, do, hip_device), S.cast_ref(x, do), f'{di}->{do} n={n}')


@pytest.mark.parametrize('di,do', S.REFUSED_PAIRS, ids=['-'.join(p) for p in S.REFUSED_PAIRS])
def test_unsupported_pairs_are_refused(hip_device, di, do):
    """bf16 <-> fp16 raises through N.call at all three entry points and leaves the destination as it was"""
    n, h, w = S.LAYOUT_NHW
    keep = torch.full((n, h, w, 8), 7.0, dtype=_dt(do))
    for entry, src_shape, dims in (('ssseg_nchw_to_nhwc', (n, 3, h, w), (n, 3, h, w)),
                                   ('ssseg_nhwc_to_nchw', (n, h, w, 8), (n, 8, h, w))):
        x, y = S.values(src_shape, di).to(hip_device), keep.to(hip_device)
        with pytest.raises(RuntimeError, match='SSSEG_EUNSUPPORTED'):
            _convert(entry, x, y, dims, 8, di, do)
        torch.cuda.synchronize()
        S.same_bits_nan(y.cpu(), keep, entry)
    N = _N()
    x, y = S.values((257,), di).to(hip_device), keep.to(hip_device)
    with pytest.raises(RuntimeError, match='SSSEG_EUNSUPPORTED'):
        N.call('ssseg_cast', x.data_ptr(), y.data_ptr(), 257, S.DT_CODE[di], S.DT_CODE[do], N.stream())
    torch.cuda.synchronize()
    S.same_bits_nan(y.cpu(), keep, 'ssseg_cast')


# ---------------------------------------------------------------------------------------------------------------------
# clip + SGD
# ---------------------------------------------------------------------------------------------------------------------
def _sgd_run(dev, op, mom, wd, max_norm, amp, first, shadow, sq_value=None):
    """one ssseg_sqnorm_accum + ssseg_sgd_step on the flat operands; returns (before, after) as host arrays"""
    o = _ops()
    n = op['p'].size
    p, g = torch.from_numpy(op['p']).to(dev), torch.from_numpy(op['g']).to(dev)
    buf = torch.from_numpy(op['buf']).to(dev) if mom != 0 else None
    sh = torch.from_numpy(op['buf']).to(dev).to(torch.bfloat16) if shadow else None   # (any content: it is overwritten)
    sq = torch.zeros(1, device=dev)
    o.sqnorm_(g, sq)
    if sq_value is not None:
        sq.fill_(sq_value)
    state = torch.tensor([op['S'], 0.0, 0.0, 1.0 / op['S']], dtype=torch.float32, device=dev) if amp else None

    def host():
        return {'p': _np(p).copy(), 'g': _np(g).copy(), 'buf': _np(buf).copy() if buf is not None else None,
                'shadow': _u16(sh).copy() if sh is not None else None}
    before = host()
    o.sgd_step_(p, g, buf, sh, S.SGD_LR, mom, wd, max_norm, sq, first, state)
    torch.cuda.synchronize()
    assert p.numel() == n
    return before, host()


@pytest.mark.parametrize('amp', S.SGD_AMP, ids=['noamp', 'amp'])
@pytest.mark.parametrize('clip', S.SGD_CLIP)
def test_sgd_step_full_cross(hip_device, clip, amp):
    """momentum x weight decay x first x shadow (16 combinations) per clip and loss-scale setting at n = 1027: the
    coefficient probe and the bit comparison of exact_step.sgd_check"""
    op = S.sgd_operands(S.SGD_N, amp)
    mx = S.sgd_max_norm(op, clip)
    for mom in S.SGD_MOM:
        for wd in S.SGD_WD:
            for first in (1, 0):
                for shadow in (False, True):
                    _, got = _sgd_run(hip_device, op, mom, wd, mx, amp, first, shadow)
                    S.sgd_check(got, op, mom, wd, mx, amp, first,
                                f'sgd clip={clip} amp={amp} mom={mom} wd={wd} first={first} shadow={shadow}')


@pytest.mark.parametrize('n', S.SGD_SIZES)
def test_sgd_step_sizes(hip_device, n):
    """one element, a workgroup less one / plus one, and the second sweep, with everything on"""
    assert S.SGD_SIZES[-1] > S.SWEEP_SGD
    op = S.sgd_operands(n, True)
    mx = S.sgd_max_norm(op, 'below')
    for first in (1, 0):
        _, got = _sgd_run(hip_device, op, 0.9, 5e-4, mx, True, first, True)
        S.sgd_check(got, op, 0.9, 5e-4, mx, True, first, f'sgd n={n} first={first}')


@pytest.mark.parametrize('sq', (float('inf'), NAN), ids=['inf', 'nan'])
def test_sgd_step_skips_a_non_finite_norm(hip_device, sq):
    """with a loss-scale state, a non-finite squared norm (set in the one-element tensor; the gradients are finite)
    leaves p, g, buf and the shadow bit-identical"""
    op = S.sgd_operands(S.SGD_N, True)
    before, after = _sgd_run(hip_device, op, 0.9, 5e-4, S.sgd_max_norm(op, 'below'), True, 0, True, sq_value=sq)
    for k in ('p', 'g', 'buf', 'shadow'):
        S.same_bits(after[k], before[k], f'skip {k}')
    S.same_bits(before['p'], op['p'], 'p upload')


# ---------------------------------------------------------------------------------------------------------------------
# squared norm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', S.SQ_SIZES)
def test_sqnorm(hip_device, n):
    """Tier A: integer data, out is the exact integer sum, and a second call ADDS the second buffer's.  Tier B: random
    data within exact_step.sq_check_bounded."""
    o = _ops()
    a, b = S.sq_ints(n, 0), S.sq_ints(n, 1)
    out = torch.zeros(1, device=hip_device)
    o.sqnorm_(torch.from_numpy(a).to(hip_device), out)
    sa = float(np.sum(a.astype(np.float64) ** 2))
    S.same_bits(_np(out), np.array([sa], np.float32), f'sqnorm n={n}')
    o.sqnorm_(torch.from_numpy(b).to(hip_device), out)
    S.same_bits(_np(out), np.array([sa + float(np.sum(b.astype(np.float64) ** 2))], np.float32), f'sqnorm += n={n}')
    x = S.sq_normals(n)
    out = torch.zeros(1, device=hip_device)
    o.sqnorm_(torch.from_numpy(x).to(hip_device), out)
    S.sq_check_bounded(_np(out)[0], x, f'sqnorm random n={n}')


# ---------------------------------------------------------------------------------------------------------------------
# EMA
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', S.EMA_ALPHAS)
@pytest.mark.parametrize('n', S.EMA_SIZES)
def test_ema(hip_device, n, alpha):
    """n < 4, the n % 4 scalar tail, and a size whose float4 loop takes a second grid-stride iteration (n / 4 > 2048 *
    256 threads) with a 3-element tail behind it"""
    e, p = S.ema_operands(n)
    ed, pd = torch.from_numpy(e).to(hip_device), torch.from_numpy(p).to(hip_device)
    _ops().ema_update_(ed, pd, alpha)
    torch.cuda.synchronize()
    S.ema_check(_np(ed), e, p, alpha, f'ema n={n} alpha={alpha}')
    S.same_bits(_np(pd), p, 'ema: the parameters')


@pytest.mark.parametrize('which', ('ema', 'param'))
def test_ema_refuses_a_misaligned_view(hip_device, which):
    """a view 4 bytes past a 16-byte boundary: N.call raises and the data is untouched"""
    n = 1023
    e, p = S.ema_operands(n)
    base = torch.zeros(n + 4, device=hip_device)
    assert base.data_ptr() % 16 == 0
    view = base[1:n + 1]
    view.copy_(torch.from_numpy(e if which == 'ema' else p))
    other = torch.from_numpy(p if which == 'ema' else e).to(hip_device)
    ed, pd = (view, other) if which == 'ema' else (other, view)
    with pytest.raises(RuntimeError, match='SSSEG_EINVAL'):
        _ops().ema_update_(ed, pd, 0.99)
    torch.cuda.synchronize()
    S.same_bits(_np(ed), e, 'ema untouched')
    S.same_bits(_np(pd), p, 'param untouched')


# ---------------------------------------------------------------------------------------------------------------------
# loss scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('growth', S.AMP_GROWTHS)
def test_amp_update_scripted_sequence(hip_device, growth):
    """exact_step.AMP_SCRIPT through amp.GradScaler.update, one launch per step: the whole state vector after every
    step equals amp_ref (the growth counter, the reset on overflow, the floor, the 1 / S slot)"""
    from ssseg import amp
    sc = amp.GradScaler(hip_device, init_scale=S.AMP_INIT, growth_factor=growth, backoff_factor=S.AMP_BACKOFF,
                        growth_interval=S.AMP_INTERVAL)
    S.same_bits(_np(sc.state), S.amp_initial(), 'initial state')
    sq = torch.zeros(1, device=hip_device)
    for i, (v, want) in enumerate(zip(S.AMP_SCRIPT, S.amp_script(growth))):
        sq.fill_(v)
        sc.update(sq)
        torch.cuda.synchronize()
        S.same_bits(_np(sc.state), want, f'amp growth={growth} step {i} (sqnorm {v})')


@pytest.mark.parametrize('n', S.SCALE_N)
def test_scale_by(hip_device, n):
    N = _N()
    x = S.vec(n, 'scale-by')
    s = np.float32(4096.0 / 3.0)
    state = torch.tensor([s, 0.0, 0.0, 1.0 / s], dtype=torch.float32, device=hip_device)
    xd = torch.from_numpy(x).to(hip_device)
    y = torch.full_like(xd, NAN)
    N.call('ssseg_scale_by', xd.data_ptr(), state.data_ptr(), y.data_ptr(), n, N.stream())
    torch.cuda.synchronize()
    S.same_bits(_np(y), S.scale_ref(x, _np(state)[0]), f'scale_by n={n}')


# ---------------------------------------------------------------------------------------------------------------------
# axpby / scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', S.AXPBY_N)
def test_axpby(hip_device, n):
    o, N = _ops(), _N()
    x, y = S.vec(n, 'x'), S.vec(n, 'y')
    xd, yd = torch.from_numpy(x).to(hip_device), torch.from_numpy(y).to(hip_device)
    for a, b in S.AXPBY_AB:
        S.same_bits(_np(o._axpby(xd, a, yd, b)), S.axpby_ref(x, a, y, b), f'axpby n={n} a={a} b={b}')
    for a in S.AXPBY_A:
        S.same_bits(_np(o._axpby(xd, a)), S.axpby_ref(x, a), f'axpby n={n} a={a}')
    # nn.replay_held's form: grad += tmp with out == x
    want = _np(o._axpby(xd, 1.0, yd, 1.0))
    N.call('ssseg_axpby', xd.data_ptr(), 1.0, yd.data_ptr(), 1.0, xd.data_ptr(), n, N.stream())
    torch.cuda.synchronize()
    S.same_bits(_np(xd), want, f'axpby in place n={n}')
    S.same_bits(want, x + y, f'axpby in place n={n}: the fp32 sum')


def test_scale_and_add_scaled_autograd(hip_device):
    """ops.scale / ops.add_scaled forward and backward: a x (+ b y) by the restatement, gradients a g and b g"""
    o = _ops()
    n = 257
    x, y, g = S.vec(n, 'x'), S.vec(n, 'y'), S.vec(n, 'g')
    gd = torch.from_numpy(g).to(hip_device)
    for a in S.AXPBY_A:
        xd = torch.from_numpy(x).to(hip_device).requires_grad_(True)
        out = o.scale(xd, a)
        out.backward(gd)
        S.same_bits(_np(out), S.axpby_ref(x, a), f'scale a={a}')
        S.same_bits(_np(xd.grad), S.axpby_ref(g, a), f'scale a={a}: gradient')
    for b in (1.0, 10.0, 0.7):
        xd = torch.from_numpy(x).to(hip_device).requires_grad_(True)
        yd = torch.from_numpy(y).to(hip_device).requires_grad_(True)
        out = o.add_scaled(xd, yd, b)
        out.backward(gd)
        S.same_bits(_np(out), S.axpby_ref(x, 1.0, y, b), f'add_scaled b={b}')
        S.same_bits(_np(xd.grad), g, f'add_scaled b={b}: dx')
        S.same_bits(_np(yd.grad), S.axpby_ref(g, b), f'add_scaled b={b}: dy')


@pytest.mark.parametrize('n', S.SCALE_F32_N)
def test_scale_f32(hip_device, n):
    """the DDP average: x *= float32(1 / 3) in place"""
    N = _N()
    x = S.vec(n, 'scale-f32')
    xd = torch.from_numpy(x).to(hip_device)
    N.call('ssseg_scale_f32', xd.data_ptr(), n, 1.0 / 3.0, N.stream())
    torch.cuda.synchronize()
    S.same_bits(_np(xd), S.scale_ref(x, np.float32(1.0 / 3.0)), f'scale_f32 n={n}')


# ---------------------------------------------------------------------------------------------------------------------
# sigmoid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', S.SIGMOID_N)
def test_sigmoid(hip_device, n):
    """ops.sigmoid forward and backward within the per-element bounds of exact_step.sigmoid_check_fwd / _bwd"""
    x, gy = S.sigmoid_operands(n)
    xd = torch.from_numpy(x).to(hip_device).requires_grad_(True)
    y = _ops().sigmoid(xd)
    y.backward(torch.from_numpy(gy).to(hip_device))
    torch.cuda.synchronize()
    v = _np(y)
    S.sigmoid_check_fwd(v, x, f'sigmoid n={n}')
    S.sigmoid_check_bwd(_np(xd.grad), v, gy, f'sigmoid backward n={n}')


# ---------------------------------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('shape', S.MIX_SHAPES, ids=['small', 'second-sweep'])
def test_mix(hip_device, shape, mode):
    """[B, 1, H, W] mask broadcast over C = 3 channels of B = 2 images in fp32, bf16 and fp16: a binary mask selects
    bit for bit, a soft one stays within exact_step.mix_check_soft"""
    assert shape == S.MIX_SHAPES[0] or int(np.prod(shape)) > S.SWEEP_DEFAULT
    o = _ops()
    a, b, m = S.mix_operands(shape, mode, False)
    got = o.mix(a.to(hip_device), b.to(hip_device), m.to(hip_device))
    S.mix_check_binary(got.cpu(), a, b, m, f'mix {mode} binary')
    a, b, m = S.mix_operands(shape, mode, True)
    got = o.mix(a.to(hip_device), b.to(hip_device), m.to(hip_device))
    S.mix_check_soft(got.cpu(), a, b, m, mode, f'mix {mode} soft')
