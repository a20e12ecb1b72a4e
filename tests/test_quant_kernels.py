"""The int8 inference kernels (csrc/quant.hip) against the CPU restatement (tests/quant_ref.py).

Integer accumulation is exact in any order, so the conv is compared with torch.equal on operands that differ along every
index (random integers: a swapped row / column or a permuted k cannot pass); the quantise, observer and weight kernels
are restated operation by operation in fp32 and compared bitwise; only the real-valued epilogue has a bound, the one
DESIGN.md derives from the fp32 roundings alone.  The conv's tiles are 128 pixels x 64 (Cout <= 64) or 128 channels.
"""
import ctypes
import zlib

import pytest
import torch

import quant_ref as Q

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
ACT = {None: 0, 'relu': 1, 'relu6': 2, 'leaky': 3}


def rup(c, v):
    return (c + v - 1) // v * v


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def nhwc_i8(q, dev):
    """q [N,C,H,W] integers -> device int8 [N,H,W,rup(C,16)], padding channels zero"""
    n, c, h, w = q.shape
    out = torch.zeros(n, h, w, rup(c, 16), dtype=torch.int8)
    out[..., :c] = q.permute(0, 2, 3, 1).to(torch.int8)
    return out.to(dev)


def pack_w(qw, dev):
    """qw [K,C,R,S] integers -> device int8 [rup(K,16)][R][S][rup(C,16)]"""
    k, c, r, s = qw.shape
    out = torch.zeros(rup(k, 16), r, s, rup(c, 16), dtype=torch.int8)
    out[:k, :, :, :c] = qw.permute(0, 2, 3, 1).to(torch.int8)
    return out.to(dev)


def out_hw(H, W, R, S, stride, pad, dil):
    return ((H + 2 * pad[0] - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad[1] - dil * (S - 1) - 1) // stride + 1)


def conv_i8(qd, qwd, shape, K, R, S, stride, pad, dil, dtype, slot, sw, scale=None, shift=None, residual=None,
            act=None, slope=0.0):
    """one ssseg_conv_i8_fwd launch; returns y as [N,K,OH,OW] (a view of the NHWC result)"""
    from ssseg import native as N
    n, C, H, W = shape
    dev = qd.device
    ldq = rup(C, 16)
    OH, OW = out_hw(H, W, R, S, stride, pad, dil)
    d = N.ConvDesc(N=n, H=H, W=W, C=ldq, ldx=ldq, OH=OH, OW=OW, K=K, R=R, S=S, sy=stride, sx=stride, dy=dil, dx=dil,
                   py=-pad[0], px=-pad[1], outH=OH, outW=OW, osy=1, osx=1, ooy=0, oox=0, ldy=K, ldw=R * S * ldq)
    y = torch.full((n, OH, OW, K), float('nan'), dtype=dtype, device=dev)
    res = None
    if residual is not None:
        res = residual.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    f = lambda t: t.to(torch.float32).to(dev) if t is not None else None  # noqa: E731
    slot_d, sw_d, scale_d, shift_d = f(torch.as_tensor(slot).reshape(1)), f(sw), f(scale), f(shift)
    if sw_d.numel() < rup(K, 16):
        sw_d = torch.cat([sw_d, torch.zeros(rup(K, 16) - sw_d.numel(), device=dev)])
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    ep = N.ConvEpilogue(p(scale_d), p(shift_d), p(res), K, None, ACT[act], float(slope))
    N.call('ssseg_conv_i8_fwd', p(qd), p(qwd), p(y), ctypes.byref(d), DT[dtype], p(slot_d), p(sw_d), ctypes.byref(ep),
           N.stream())
    return y.permute(0, 3, 1, 2)


def same(k, d):
    return d * (k - 1) // 2


# (Cin, Cout, N, H, W, R, S, stride, dilation, 'same' padding?)
ACC_CASES = [
    (8, 8, 1, 5, 7, 1, 1, 1, 1, False), (24, 24, 2, 9, 11, 3, 3, 1, 1, True), (64, 72, 1, 5, 7, 3, 3, 2, 1, True),
    (72, 56, 2, 9, 11, 1, 3, 1, 1, True), (200, 64, 1, 5, 7, 7, 7, 1, 1, True), (8, 120, 2, 9, 11, 7, 7, 2, 1, True),
    (24, 136, 1, 3, 43, 3, 3, 1, 2, True), (64, 24, 1, 1, 127, 1, 1, 1, 1, False), (72, 8, 2, 9, 11, 3, 3, 1, 12, True),
    (200, 72, 2, 9, 11, 1, 1, 2, 1, False), (24, 8, 2, 9, 11, 3, 3, 2, 2, False), (64, 128, 1, 3, 43, 1, 3, 2, 2, True),
    (8, 72, 1, 5, 7, 3, 3, 1, 1, False), (200, 24, 1, 1, 127, 1, 3, 1, 1, True), (72, 64, 1, 3, 43, 7, 7, 1, 2, True),
    (24, 72, 2, 9, 11, 7, 7, 1, 1, False),
]


def _geom(case):
    cin, cout, n, H, W, R, S, stride, dil, samep = case
    pad = (same(R, dil), same(S, dil)) if samep else (0, 0)
    return cin, cout, n, H, W, R, S, stride, dil, pad


@pytest.mark.parametrize('case', ACC_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_conv_accumulators_exact(hip_device, case):
    cin, cout, n, H, W, R, S, stride, dil, pad = _geom(case)
    g = gen('acc', case)
    x = torch.randint(-4, 5, (n, cin, H, W), generator=g)
    w = torch.randint(-3, 4, (cout, cin, R, S), generator=g)
    acc = F_conv(x, w, stride, pad, dil)
    assert float(acc.abs().max()) < 2 ** 24 and float((acc != 0).double().mean()) > 0.5
    y = conv_i8(nhwc_i8(x, hip_device), pack_w(w, hip_device), x.shape, cout, R, S, stride, pad, dil, torch.float32,
                127.0, torch.ones(cout))
    assert y.shape == acc.shape
    got = y.cpu()
    if not torch.equal(got, acc.float()):
        bad = (got != acc.float()).nonzero()
        print(f'{bad.shape[0]} of {got.numel()} differ; first (n,k,oy,ox):', bad[:8].tolist())
    assert torch.equal(got, acc.float())


def F_conv(x, w, stride, pad, dil):
    import torch.nn.functional as F
    return F.conv2d(x.double(), w.double(), None, stride, pad, dil)


def test_conv_full_range_accumulators(hip_device):
    """operands at +-127 with R S Cin = 4608: |acc| passes 2^24, the stored value is the round-to-nearest fp32 of the
    exact integer"""
    g = gen('full')
    x = torch.randint(0, 2, (1, 512, 6, 6), generator=g) * 254 - 127
    w = torch.randint(0, 2, (16, 512, 3, 3), generator=g) * 254 - 127
    w[0] = 127 * torch.sign(x[0, :, 1:4, 1:4])          # one output sums 4608 * 127^2 = 74 322 432
    for k in range(1, 16):                              # filters matched to other patches, magnitudes 64 .. 127
        oy, ox = k // 4, k % 4
        w[k] = torch.sign(x[0, :, oy:oy + 3, ox:ox + 3]) * torch.randint(64, 128, (512, 3, 3), generator=g) \
            * (1 if k % 2 else -1)
    acc = F_conv(x, w, 1, (1, 1), 1)
    assert float(acc[0, 0, 2, 2]) == 4608 * 127 * 127 and float(acc.abs().max()) > 2 ** 24
    assert int((acc.abs() > 2 ** 24).sum()) >= 16
    assert int((acc.float().double() != acc).sum()) >= 4    # some accumulators do round
    y = conv_i8(nhwc_i8(x, hip_device), pack_w(w, hip_device), x.shape, 16, 3, 3, 1, (1, 1), 1, torch.float32, 127.0,
                torch.ones(16))
    assert torch.equal(y.cpu(), acc.float())


EXACT_BOUND = {torch.float32: 2 ** 24, torch.bfloat16: 256, torch.float16: 2048}   # tests/exact.py STORE_BOUND


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('act', [None, 'relu', 'relu6', 'leaky'])
def test_epilogue_exact(hip_device, dtype, act):
    """power-of-two scales, integer shift and residual: every fp32 operation and the store are exact"""
    slope = 2.0 ** -3
    for cin, cout, R, pad in ((24, 40, 1, 0), (8, 72, 3, 1)):
        g = gen('epi', cin, cout, R, str(dtype), act)
        x = torch.randint(-1, 2, (2, cin, 9, 11), generator=g)
        w = torch.randint(-1, 2, (cout, cin, R, R), generator=g)
        acc = F_conv(x, w, 1, (pad, pad), 1)
        # slot 254 -> sx = 2; sw in {1/2, 1}; scale in {1/2, 1, 2}: m = sx sw scale in {1/2 .. 4}
        sw = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (cout,), generator=g)]
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
        shift = torch.randint(-3, 4, (cout,), generator=g).float()
        res = torch.randint(-3, 4, acc.shape, generator=g).float()
        pre, _ = Q.epilogue(acc, 254.0, sw, scale, shift, res, None)
        v, _ = Q.epilogue(acc, 254.0, sw, scale, shift, res, act, slope)
        # the pre-activation is a multiple of 1/2 within the storage format's integer range (tests/exact.py), so the
        # fp32 fmaf and add are exact, and the activated value stores without rounding
        assert torch.equal(pre * 2, (pre * 2).round()) and float((pre * 2).abs().max()) <= EXACT_BOUND[dtype]
        assert torch.equal(v.to(dtype).double(), v)
        assert bool((pre < 0).any()) and bool((pre > 6).any())     # every activation has something to cut
        y = conv_i8(nhwc_i8(x, hip_device), pack_w(w, hip_device), x.shape, cout, R, R, 1, (pad, pad), 1, dtype,
                    254.0, sw, scale, shift, res, act, slope)
        assert torch.equal(y.cpu(), v.to(dtype)), (cin, cout)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('act', [None, 'relu', 'leaky'])
def test_epilogue_real_valued_within_bound(hip_device, dtype, act):
    """real scales, shifts and residuals, half of the outputs near cancellation:
    |y - v| <= 1/2 ulp_out(v) + 2^-21 (|acc m| + |shift| + |residual|)"""
    cin, cout, R = 72, 136, 3
    g = gen('real', str(dtype), act)
    x = torch.randint(-127, 128, (2, cin, 9, 11), generator=g)
    w = torch.randint(-127, 128, (cout, cin, R, R), generator=g)
    acc = F_conv(x, w, 1, (1, 1), 1)
    slot = torch.tensor(3.7)
    sw = torch.rand(cout, generator=g) * 0.01 + 1e-4
    scale = (torch.rand(cout, generator=g) + 0.5) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1).float()
    shift = torch.randn(cout, generator=g)
    pre, _ = Q.epilogue(acc, slot, sw, scale, shift, None, None)
    # residual: the negated pre-activation as the output dtype holds it on half of the elements (cancellation)
    near = torch.rand(acc.shape, generator=g) < 0.5
    res = torch.where(near, -pre, torch.randn(acc.shape, generator=g).double() * 4).to(dtype)
    v, mag = Q.epilogue(acc, slot, sw, scale, shift, res, act, 0.125)
    assert float((v.abs() < 0.05 * mag).double().mean()) > 0.4
    y = conv_i8(nhwc_i8(x, hip_device), pack_w(w, hip_device), x.shape, cout, R, R, 1, (1, 1), 1, dtype, slot, sw,
                scale, shift, res, act, 0.125)
    Q.assert_within(y.cpu(), v, mag, dtype, 'real-valued epilogue')


# ---- quantise ------------------------------------------------------------------------------------------------------
def quantize_dev(x, C, slot, dev):
    """x [P, ldx] (any float dtype, host) -> int8 [P, rup(C,16)] from the device"""
    from ssseg import native as N
    xd = x.to(dev)
    P, ldx = x.shape
    ldq = rup(C, 16)
    q = torch.full((P, ldq), 77, dtype=torch.int8, device=dev)
    sd = torch.as_tensor(slot, dtype=torch.float32).reshape(1).to(dev)
    N.call('ssseg_quantize_i8', xd.data_ptr(), P, C, ldx, DT[x.dtype], sd.data_ptr(), q.data_ptr(), ldq, N.stream())
    return q.cpu()


def want_q(x, C, slot):
    P = x.shape[0]
    out = torch.zeros(P, rup(C, 16), dtype=torch.int8)
    out[:, :C] = Q.quantize(x[:, :C], slot)
    return out


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
def test_quantize_ties_clamp_nonfinite(hip_device, dtype):
    g = gen('q', str(dtype))
    P, C = 37, 24
    # slot 127 -> unit scale: half-integers are ties in both directions; values above the slot clamp
    x = (torch.randint(-260, 261, (P, C), generator=g).float() / 2).to(dtype)
    x[0, :6] = torch.tensor([0.5, -0.5, 2.5, -2.5, 127.5, -300.0]).to(dtype)
    x[1, :4] = torch.tensor([float('nan'), float('inf'), -float('inf'), 126.5]).to(dtype)
    got = quantize_dev(x, C, 127.0, hip_device)
    want = want_q(x, C, 127.0)
    assert want[0, :6].tolist() == [0, 0, 2, -2, 127, -127] and want[1, :4].tolist() == [0, 127, -127, 126]
    assert torch.equal(got, want)
    # a real scale, and a zero slot
    xr = (torch.randn(P, C, generator=g) * 3).to(dtype)
    assert torch.equal(quantize_dev(xr, C, 2.9, hip_device), want_q(xr, C, 2.9))
    assert torch.equal(quantize_dev(xr, C, 0.0, hip_device), torch.zeros(P, 32, dtype=torch.int8))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
def test_quantize_ignores_padding_channels(hip_device, dtype):
    """C = 8 real channels in an ldx of 16: NaN and garbage in the padding never reach q; P C is no multiple of 16"""
    g = gen('qpad', str(dtype))
    P, C, ldx = 21, 8, 16
    x = torch.randn(P, ldx, generator=g).to(dtype)
    x[:, C:] = float('nan')
    x[::2, C + 1] = 1e30
    got = quantize_dev(x, C, 1.5, hip_device)
    assert torch.equal(got, want_q(x, C, 1.5)) and int(got[:, C:].abs().sum()) == 0
    # odd widths: a ragged tail inside a 16-byte group, an unaligned pixel stride
    for C2, ld2 in ((13, 13), (20, 24), (9, 11)):
        x2 = torch.randn(P, ld2, generator=g).to(dtype)
        x2[:, C2:] = float('nan')
        assert torch.equal(quantize_dev(x2, C2, 2.0, hip_device), want_q(x2, C2, 2.0)), (C2, ld2)


def test_quantize_past_the_grid_stride_cap(hip_device):
    """2048 workgroups x 256 threads own one 16-byte chunk each per pass: a few chunks more take the second pass"""
    P, C = 2048 * 256 + 5, 16
    x = ((torch.arange(P * C, dtype=torch.float32) * 0.37) % 9.0 - 4.5).reshape(P, C).to(torch.bfloat16)
    got = quantize_dev(x, C, 4.5, hip_device)
    assert torch.equal(got, want_q(x, C, 4.5))


# ---- observer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32], ids=['bf16', 'f16', 'f32'])
def test_absmax_three_updates(hip_device, dtype):
    from ssseg import native as N
    g = gen('amax', str(dtype))
    P, C, ldx = 333, 20, 24
    xs = [torch.randn(P, ldx, generator=g).to(dtype) for _ in range(3)]
    xs[1][200, 7] = -9.25                       # the largest magnitude: negative, in the second update
    for x in xs:
        x[:, C:] = 50.0                         # padding channels are not observed
        x[5, C + 1] = float('nan')
    xs[0][3, 2] = float('nan')
    xs[2][4, 1] = float('inf')
    xs[2][9, 0] = -float('inf')
    slot = torch.zeros(1, dtype=torch.float32, device=hip_device)
    seen = []
    for x in xs:
        xd = x.to(hip_device)
        N.call('ssseg_absmax_update', xd.data_ptr(), P, C, ldx, DT[dtype], slot.data_ptr(), N.stream())
        seen.append(slot.cpu().clone())
    want = [Q.absmax(torch.stack(xs[:i + 1])[:, :, :C]) for i in range(3)]
    assert float(want[1]) == 9.25 and float(want[0]) < 9.25
    for s, w in zip(seen, want):
        assert torch.equal(s.reshape(()), w.reshape(()))
    # an unaligned pixel stride, one pixel
    x1 = torch.randn(1, 9, generator=g).to(dtype)
    slot.zero_()
    x1d = x1.to(hip_device)
    N.call('ssseg_absmax_update', x1d.data_ptr(), 1, 7, 9, DT[dtype], slot.data_ptr(), N.stream())
    assert torch.equal(slot.cpu().reshape(()), Q.absmax(x1[:, :7]).reshape(()))


# ---- weights -------------------------------------------------------------------------------------------------------
def test_weight_quant_through_a_conv(hip_device):
    """sw is bitwise amax / 127; the packed layout [Kp][R][S][Cq] is what the conv reads: checked through its result"""
    from ssseg import native as N
    g = gen('wq')
    K, C, R, S = 24, 20, 3, 2
    w = torch.randn(K, C, R, S, generator=g)
    w[3] = 0.0                                                       # an all-zero channel
    w[5] = torch.randint(-254, 255, (C, R, S), generator=g).float() / 2  # ties: amax 127 makes the scale 1
    w[5, 0, 0, 0] = 127.0
    Kp, Cq = rup(K, 16), rup(C, 16)
    wd = w.to(hip_device)
    qwd = torch.full((Kp * R * S * Cq,), 77, dtype=torch.int8, device=hip_device)
    swd = torch.full((Kp,), 77.0, dtype=torch.float32, device=hip_device)
    N.call('ssseg_weight_quant_i8', wd.data_ptr(), K, C, R, S, Kp, Cq, qwd.data_ptr(), swd.data_ptr(), N.stream())
    qw, sw = Q.weight_quant(w)
    assert float(sw[3]) == 0.0 and float(sw[5]) == 1.0 and int((w[5] * 2 % 2 == 1).sum()) > 20   # ties present
    assert torch.equal(swd.cpu()[:K], sw) and float(swd.cpu()[K:].abs().sum()) == 0.0
    assert torch.equal(swd.cpu()[:K], w.abs().amax((1, 2, 3)) / 127.0)
    x = torch.randint(-127, 128, (2, C, 9, 11), generator=g)
    acc = F_conv(x, qw, 1, (1, 0), 1)
    assert float(acc.abs().max()) < 2 ** 24
    y = conv_i8(nhwc_i8(x, hip_device), qwd, x.shape, K, R, S, 1, (1, 0), 1, torch.float32, 127.0, swd)
    # unit sx: y = fp32(acc * sw), one rounding
    want = (acc * sw.double().view(1, K, 1, 1)).float()
    assert torch.equal(y.cpu(), want)
    assert int(y.cpu()[:, 3].abs().sum()) == 0
