"""Host-side tests of the int8 inference feature: the restatement's own properties, the new entry points' argument
checks (refused on the host, no device touched), and prepare / summary / state_dict on a CPU-constructed model."""
import ctypes

import pytest
import torch

import quant_ref as Q


def test_restatement_rounds_ties_to_even_and_clamps():
    a = torch.tensor(127.0)   # unit scale: q = rint(x)
    x = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.49, 126.5, 127.5, 300.0, -300.0])
    assert Q.quantize(x, a).tolist() == [0, 2, 2, 0, -2, -2, 3, 126, 127, 127, -127]
    # 16-bit inputs are widened first
    assert Q.quantize(torch.tensor([2.5, -3.5], dtype=torch.bfloat16), a).tolist() == [2, -4]
    assert Q.quantize(torch.tensor([2.5, -3.5], dtype=torch.float16), a).tolist() == [2, -4]


def test_restatement_zero_scale_and_non_finite():
    x = torch.tensor([1.0, float('nan'), float('inf'), -float('inf'), -4.0])
    assert Q.quantize(x, torch.tensor(0.0)).tolist() == [0, 0, 0, 0, 0]
    assert Q.quantize(x, torch.tensor(4.0)).tolist() == [32, 0, 127, -127, -127]
    assert float(Q.absmax(x)) == 4.0 and float(Q.absmax(torch.tensor([float('nan'), float('inf')]))) == 0.0
    # the largest magnitude is negative
    assert float(Q.absmax(torch.tensor([1.0, -7.5, 3.0]))) == 7.5


def test_restatement_weight_quant():
    w = torch.zeros(3, 2, 1, 2)
    w[0] = torch.tensor([[[127.0, 0.5]], [[-1.5, 2.5]]])     # amax 127: unit scale, ties
    w[2] = torch.tensor([[[0.25, -0.5]], [[0.125, 0.0]]])    # amax 0.5: scale 254
    qw, sw = Q.weight_quant(w)
    assert qw[0].flatten().tolist() == [127, 0, -2, 2]
    assert qw[1].abs().sum() == 0 and float(sw[1]) == 0.0      # an all-zero channel
    assert qw[2].flatten().tolist() == [64, -127, 32, 0]       # 63.5 -> 64 (even)
    assert torch.equal(sw, torch.tensor([127.0, 0.0, 0.5]) / torch.tensor(127.0))


def test_restatement_conv_and_epilogue():
    g = torch.Generator().manual_seed(0)
    q = torch.randint(-127, 128, (1, 8, 5, 7), generator=g)
    qw = torch.randint(-127, 128, (8, 8, 3, 3), generator=g)
    acc = Q.conv_acc(q, qw, 1, 1, 1)
    want = sum(int(q[0, c, 1 + r - 1, 2 + s - 1]) * int(qw[3, c, r, s]) for c in range(8) for r in range(3)
               for s in range(3))
    assert float(acc[0, 3, 1, 2]) == want
    sw = torch.full((8,), 1.0 / 127.0)
    v, mag = Q.epilogue(acc, torch.tensor(127.0), sw * 127, None, torch.arange(8.0), None, 'relu')
    assert torch.equal(v, (acc + torch.arange(8.0).double().view(1, 8, 1, 1)).clamp(min=0))
    assert torch.equal(mag, acc.abs() + torch.arange(8.0).double().view(1, 8, 1, 1))
    assert float(Q.ulp(torch.tensor(1.5, dtype=torch.float64), torch.bfloat16)) == 2.0 ** -7
    assert float(Q.ulp(torch.tensor(4.0, dtype=torch.float64), torch.float16)) == 2.0 ** -8
    assert float(Q.ulp(torch.tensor(0.0, dtype=torch.float64), torch.float32)) == 2.0 ** -149


def test_entry_points_are_declared_and_refuse_null_pointers():
    from ssseg import native
    new = {'ssseg_absmax_update', 'ssseg_quantize_i8', 'ssseg_weight_quant_i8', 'ssseg_conv_i8_fwd'}
    assert new <= set(native.header_symbols()) and new <= set(native.SIGS)
    lib = native.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: a NULL among the others is refused first
    assert lib.ssseg_absmax_update(None, 4, 8, 8, native.BF16, one, None) == -1
    assert lib.ssseg_absmax_update(one, 4, 8, 8, native.BF16, None, None) == -1
    assert lib.ssseg_quantize_i8(None, 4, 8, 8, native.BF16, one, one, 16, None) == -1
    assert lib.ssseg_quantize_i8(one, 4, 8, 8, native.BF16, None, one, 16, None) == -1
    assert lib.ssseg_quantize_i8(one, 4, 8, 8, native.BF16, one, None, 16, None) == -1
    assert lib.ssseg_quantize_i8(one, 4, 8, 8, native.BF16, one, one, 8, None) == -1      # ldq != rup(C, 16)
    assert lib.ssseg_weight_quant_i8(None, 8, 8, 3, 3, 16, 16, one, one, None) == -1
    assert lib.ssseg_weight_quant_i8(one, 8, 8, 3, 3, 16, 16, None, one, None) == -1
    assert lib.ssseg_weight_quant_i8(one, 8, 8, 3, 3, 16, 16, one, None, None) == -1
    assert lib.ssseg_weight_quant_i8(one, 8, 8, 3, 3, 16, 8, one, one, None) == -1        # Cq % 16
    d = native.ConvDesc(N=1, H=5, W=7, C=16, ldx=16, OH=5, OW=7, K=8, R=3, S=3, sy=1, sx=1, dy=1, dx=1, py=-1, px=-1,
                        outH=5, outW=7, osy=1, osx=1, ooy=0, oox=0, ldy=8, ldw=144)
    ok = [one, one, one, ctypes.byref(d), native.F32, one, one, None, None]
    for i in (0, 1, 2, 3, 5, 6):
        args = list(ok)
        args[i] = None
        assert lib.ssseg_conv_i8_fwd(*args) == -1
    # aux / stats are not part of the int8 epilogue
    ep = native.ConvEpilogue(None, None, None, 0, one, 1, 0.0)
    assert lib.ssseg_conv_i8_fwd(*ok[:7], ctypes.byref(ep), None) == -1
    # geometry outside the kernel: the library's "unsupported" status, before any launch
    for field, val in (('R', 9), ('sy', 3), ('C', 24), ('K', 12), ('osy', 2), ('ldw', 100)):
        bad = native.ConvDesc.from_buffer_copy(d)
        setattr(bad, field, val)
        args = list(ok)
        args[3] = ctypes.byref(bad)
        assert lib.ssseg_conv_i8_fwd(*args) == native.EUNSUPPORTED, field


def _unet_r50():
    from models import unet
    from models.encoders import resnet
    return unet.UNet(2, resnet.resnet50_encoder(), 128, train_upsampling=True)


def test_prepare_summary_state_dict_on_a_cpu_model():
    from ssseg import nn as snn
    from ssseg import quant
    m = _unet_r50().eval()
    with pytest.raises(RuntimeError):
        quant.state_dict(m)                       # not prepared
    before = {r['name']: r for r in quant.summary(m)}
    assert not any(r['int8'] for r in before.values())
    assert quant.prepare(m) is m and quant.prepare(m) is m
    rows = {r['name']: r for r in quant.summary(m)}
    convs = {n: c for n, c in m.named_modules() if isinstance(c, (snn.Conv2d, snn.ConvTranspose2d))}
    assert set(rows) == set(convs)
    # never int8: the image stem, the fp32 head, the transposed upsamplers
    stems = [n for n, c in convs.items() if c.in_channels == 3]
    assert len(stems) == 1 and 'stem' in rows[stems[0]]['reason'] and 'head' in rows['final_block']['reason']
    ups = [n for n, c in convs.items() if isinstance(c, snn.ConvTranspose2d)]
    assert ups and all(rows[n]['reason'] == 'ConvTranspose2d' for n in ups)
    # eligible, waiting for calibration
    elig = [n for n, c in convs.items() if '_ssseg_q' in c.__dict__]
    assert any(n.startswith('encoder') and n.endswith('conv2') for n in elig)     # Bottleneck 3x3
    assert any(n.startswith('decoder') and 'conv3_0' in n for n in elig)          # decoder ConvBlock
    assert all(rows[n]['reason'] == 'not calibrated' and not rows[n]['int8'] for n in elig)
    assert len(elig) + len(ups) + 2 == len(convs)
    assert quant.state_dict(m) == {}
    # a state restores the slots and converts: those convs now report int8
    state = {n: torch.tensor(1.0 + i) for i, n in enumerate(elig[:3])}
    quant.load_state_dict(m, state, rule='all')
    got = quant.state_dict(m)
    assert set(got) == set(state) and all(torch.equal(got[n], state[n]) for n in state)
    rows = {r['name']: r for r in quant.summary(m)}
    assert all(rows[n]['int8'] and rows[n]['reason'] is None for n in elig[:3])
    assert all(not rows[n]['int8'] for n in elig[3:])
    # the default rule keeps a class that measured slower in int8 in the 16-bit path, and says so
    quant.convert(m)
    for n in elig[:3]:
        c = convs[n]
        worth = quant.worth_int8(c.kernel_size[0] * c.kernel_size[1] * c.in_channels, c.out_channels)
        r = {x['name']: x for x in quant.summary(m)}[n]
        assert r['int8'] == worth and (worth or 'measured rule' in r['reason'])
    assert quant.worth_int8(1, 8, 'all') and quant.state_dict(m).keys() == state.keys()
    with pytest.raises(ValueError):
        quant.convert(m, rule='fastest')
    with pytest.raises(KeyError):
        quant.load_state_dict(m, {'no.such.conv': torch.tensor(1.0)})
    m.train()
    with pytest.raises(RuntimeError):
        quant.convert(m)
    with pytest.raises(RuntimeError):
        quant.quantized(m)


def test_depthwise_is_reported_bf16():
    from models import unet
    from models.encoders import mobilenetv2
    from ssseg import quant
    m = unet.UNet(2, mobilenetv2.mobilenet_v2(width_mult=0.35), 32, train_upsampling=True).eval()
    quant.prepare(m)
    reasons = {r['reason'] for r in quant.summary(m)}
    assert 'depthwise' in reasons and 'not calibrated' in reasons
