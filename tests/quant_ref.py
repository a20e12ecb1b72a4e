"""Pure-torch CPU restatement of the int8 inference scheme (include/ssseg.h "Post-training int8 inference").

quantize / weight_quant restate the device arithmetic in fp32, operation by operation, so their results are compared
with torch.equal.  conv_acc is the integer convolution as an fp64 F.conv2d: exact, because |acc| <= 127^2 R S Cin is far
below 2^53.  epilogue evaluates the scheme's epilogue in fp64 from the fp32 inputs; epilogue_bound is the per-element
error bound of the device's fp32 evaluation against it (derived in DESIGN.md):

    |y - v| <= 1/2 ulp_out(v) + 2^-21 (|acc m| + |shift| + |residual|)
"""
import torch
import torch.nn.functional as F

F32 = torch.float32
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def inv_scale(a):
    """127.0f / a in fp32 (0 where a is not positive)"""
    a = torch.as_tensor(a, dtype=F32)
    return torch.where(a > 0, torch.tensor(127.0, dtype=F32) / a, torch.zeros((), dtype=F32))


def _rint_clamp(t):
    """rint (ties to even), NaN -> 0, clamp to [-127, 127] (so +-Inf -> +-127)"""
    t = torch.where(torch.isnan(t), torch.zeros((), dtype=F32), t)
    return torch.round(t).clamp(-127, 127).to(torch.int8)


def quantize(x, a):
    """int8 of x (any float dtype, any shape) under the slot value a: clamp(rint(float(x) * (127.0f / a)), -127, 127)"""
    a = torch.as_tensor(a, dtype=F32).reshape(())
    if not bool(a > 0):
        return torch.zeros(x.shape, dtype=torch.int8)
    return _rint_clamp(x.detach().cpu().to(F32) * inv_scale(a))


def absmax(x):
    """max over the finite |x| (0 if there is none), fp32"""
    v = x.detach().cpu().to(F32).abs().flatten()
    v = v[torch.isfinite(v)]
    return v.max() if v.numel() else torch.zeros((), dtype=F32)


def weight_quant(w):
    """w [K,C,R,S] fp32 -> (qw int8 [K,C,R,S], sw fp32 [K]): per-output-channel symmetric int8"""
    w = w.detach().cpu().to(F32)
    aw = w.abs().amax((1, 2, 3))
    sw = aw / torch.tensor(127.0, dtype=F32)
    qw = _rint_clamp(w * inv_scale(aw).view(-1, 1, 1, 1))
    qw = torch.where((aw > 0).view(-1, 1, 1, 1), qw, torch.zeros((), dtype=torch.int8))
    return qw, torch.where(aw > 0, sw, torch.zeros((), dtype=F32))


def conv_acc(q, qw, stride=1, padding=0, dilation=1):
    """exact integer accumulators as fp64: q [N,C,H,W], qw [K,C,R,S] (integer-valued tensors of any dtype)"""
    return F.conv2d(q.double(), qw.double(), None, stride, padding, dilation)


def act(v, code, slope=0.0):
    """code: None | 'relu' | 'relu6' | 'leaky'"""
    if code in (None, 'none'):
        return v
    if code == 'relu':
        return v.clamp(min=0)
    if code == 'relu6':
        return v.clamp(0, 6)
    if code == 'leaky':
        return torch.where(v > 0, v, v * slope)
    raise ValueError(code)


def epilogue(acc, a, sw, scale=None, shift=None, residual=None, code=None, slope=0.0):
    """fp64 value v = act(acc * m + shift + residual) with m = sx * sw[k] * scale[k] from the fp32 inputs
    (sx = a / 127.0f in fp32, as the scheme defines it), and the bound's magnitude |acc m| + |shift| + |residual|.
    acc [N,K,OH,OW] fp64; sw / scale / shift [K]; residual like acc."""
    K = acc.shape[1]
    sx = (torch.as_tensor(a, dtype=F32).reshape(()) / torch.tensor(127.0, dtype=F32)).double()
    m = sx * sw.detach().cpu().double()[:K]
    if scale is not None:
        m = m * scale.detach().cpu().double()[:K]
    sh = shift.detach().cpu().double()[:K] if shift is not None else torch.zeros(K, dtype=torch.float64)
    res = residual.detach().cpu().double() if residual is not None else torch.zeros_like(acc)
    am = acc * m.view(1, K, 1, 1)
    v = act(am + sh.view(1, K, 1, 1) + res, code, slope)
    mag = am.abs() + sh.abs().view(1, K, 1, 1) + res.abs()
    return v, mag


def ulp(v, dtype):
    """spacing of `dtype` at |v| (fp64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** EMIN[dtype]))).clamp(min=EMIN[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def epilogue_bound(v, mag, dtype):
    return 0.5 * ulp(v, dtype) + 2.0 ** -21 * mag


def assert_within(y, v, mag, dtype, what):
    """every element of the device result y (dtype) within epilogue_bound of the fp64 value v"""
    err = (y.detach().cpu().double() - v).abs()
    bound = epilogue_bound(v, mag, dtype)
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first {i}: '
                             f'got {float(y[i])} want {float(v[i])} err {float(err[i])} bound {float(bound[i])}')
