"""ssseg.quant on real models: UNet over the ResNet-50 encoder (residual joins, strided downsample convs, the decoder's
concat) and the dilated DeepLabV3-R50, at 64 x 64.  Every quantised launch of the real forward is checked at its real
geometry against the CPU restatement (tests/quant_ref.py): the int8 input bitwise, the output within the epilogue's
fp32-rounding bound.  No tolerance is measured."""
import io
import json
import os
import subprocess
import sys

import pytest
import torch

import quant_ref as Q
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ACT_NAME = {0: None, 1: 'relu', 2: 'relu6', 3: 'leaky'}


def _randomize_bn(model, seed):
    """non-trivial folds: random running statistics, gamma (both signs) and beta"""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.25)
            with torch.no_grad():
                m.weight.copy_((torch.rand(n, generator=g) * 0.9 + 0.4) * (torch.randint(0, 8, (n,), generator=g) > 0)
                               .float().mul(2).sub(1))
                m.bias.copy_(torch.randn(n, generator=g) * 0.3)


def _build(kind, seed=0):
    from models import deeplabv3, unet
    from models.adapters import ListOutput
    from models.encoders import resnet
    torch.manual_seed(seed)
    if kind == 'unet':
        net = ListOutput(unet.UNet(2, resnet.resnet50_encoder(), 128, train_upsampling=True))
    else:
        net = deeplabv3.deeplabv3_resnet50(2)
    _randomize_bn(net, seed + 1)
    return net.eval()


def _logits(out):
    if isinstance(out, (tuple, list)) and len(out) == 2 and isinstance(out[1], (list, tuple)):
        return out[1][-1]
    if isinstance(out, dict):
        return out['out']
    return out


class State:
    pass


def _prepare(kind, dev, batch):
    from ssseg import quant
    st = State()
    st.model = _build(kind).to(dev)
    g = torch.Generator().manual_seed(7)
    st.x = [torch.rand(batch, 3, 64, 64, generator=g).to(dev) for _ in range(3)]
    with torch.no_grad():
        st.before = _logits(st.model(st.x[2])).clone()
    quant.prepare(st.model)
    with quant.trace() as st.cal_rows, quant.calibrating(st.model):
        st.model(st.x[0])
        st.model(st.x[1])
    quant.convert(st.model, rule='all')
    with torch.no_grad():
        st.after_convert = _logits(st.model(st.x[2])).clone()
    with quant.trace() as st.rows, quant.quantized(st.model):
        st.yq = _logits(st.model(st.x[2])).clone()
    with torch.no_grad():
        st.after = _logits(st.model(st.x[2])).clone()
    torch.cuda.synchronize()
    return st


@pytest.fixture(scope='module')
def unet_state(hip_device):
    return _prepare('unet', hip_device, 2)


@pytest.fixture(scope='module')
def deeplab_state(hip_device):
    return _prepare('deeplab', hip_device, 1)


def _check_calibration(st):
    from ssseg import quant
    by_conv = {}
    for r in st.cal_rows:
        assert r['mode'] == 'calibrate'
        C = r['conv'].in_channels
        by_conv.setdefault(r['conv'], []).append(Q.absmax(r['input'][:, :C]))
    recs = st.model.__dict__['_ssseg_quant_recs']
    assert by_conv and set(by_conv) == {rec.conv for rec in recs if rec.seen}
    assert all(len(v) >= 2 for v in by_conv.values())     # both batches
    state = quant.state_dict(st.model)
    for rec in recs:
        if rec.seen:
            want = torch.stack(by_conv[rec.conv]).max()
            assert torch.equal(rec.slot.cpu().reshape(()), want), rec.name
            assert torch.equal(state[rec.name], want) and float(want) > 0


def _check_launches(st):
    from ssseg import nn as snn
    assert st.rows and all(r['mode'] == 'int8' for r in st.rows)
    wq = {}
    for r in st.rows:
        conv = r['conv']
        rec = conv.__dict__['_ssseg_q']
        C, K = conv.in_channels, conv.out_channels
        x, q, y = r['input'], r['q'].cpu(), r['output']
        slot = rec.slot.cpu().reshape(())
        # the int8 input: the restated quantise of the traced input, zero padding
        assert torch.equal(q[..., :C], Q.quantize(x[:, :C].permute(0, 2, 3, 1), slot)), rec.name
        assert int(q[..., C:].abs().sum()) == 0
        if conv not in wq:
            wq[conv] = Q.weight_quant(conv.weight)
        qw, sw = wq[conv]
        acc = Q.conv_acc(q[..., :C].permute(0, 3, 1, 2), qw, conv.stride, conv.padding, conv.dilation)
        code, slope = snn._act(r['act'])
        res = r['residual'][:, :K] if r['residual'] is not None else None
        bn = r['bn']
        if bn is not None:   # the frozen fold belongs to this BN: scale = gamma / sqrt(var + eps)
            want = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu()
            assert torch.allclose(r['scale'][:K].double().cpu(), want, rtol=1e-5, atol=0)
        v, mag = Q.epilogue(acc, slot, sw, r['scale'], r['shift'], res, ACT_NAME[code], slope)
        assert y.shape[1] >= K and tuple(y.shape[2:]) == tuple(v.shape[2:])
        Q.assert_within(y[:, :K].cpu(), v, mag, y.dtype, rec.name)
        assert float(y[:, K:].float().abs().sum()) == 0.0
        assert float((v != 0).double().mean()) > 0.05, rec.name    # a live layer, not a zero map
    return wq


def test_unet_calibration_slots_are_the_traced_amax(unet_state):
    _check_calibration(unet_state)


def test_unet_every_quantised_launch_matches_the_restatement(unet_state):
    st = unet_state
    _check_launches(st)
    rows = st.rows
    assert any(r['residual'] is not None for r in rows)                                    # residual joins
    assert any(r['conv'].stride == (2, 2) and r['conv'].kernel_size == (1, 1) for r in rows)   # strided downsample
    assert any(r['conv'].stride == (2, 2) and r['conv'].kernel_size == (3, 3) for r in rows)
    assert any(r['conv'].in_channels > r['conv'].out_channels and r['conv'].kernel_size == (3, 3)
               and r['bn'] is not None and r['residual'] is None and r['input'].shape[1] == r['conv'].in_channels
               and '_ssseg_materialized' in r['input'].__dict__ for r in rows)             # the materialised concat
    assert float((st.yq - st.before).abs().max()) > 0                                      # int8 did run


def test_deeplab_dilated_launches_match_the_restatement(deeplab_state):
    st = deeplab_state
    _check_calibration(st)
    _check_launches(st)
    dil = {r['conv'].dilation[0] for r in st.rows}
    assert {1, 2, 4} <= dil and max(dil) >= 12      # the dilated backbone layers and the ASPP branches


def test_summary_reports_the_dispatch(unet_state):
    from ssseg import nn as snn
    from ssseg import quant
    rows = {r['name']: r for r in quant.summary(unet_state.model)}
    mods = dict(unet_state.model.named_modules())
    for name, r in rows.items():
        m = mods[name]
        if isinstance(m, snn.ConvTranspose2d):
            assert not r['int8'] and r['reason'] == 'ConvTranspose2d'
        elif m._ssseg_head:
            assert not r['int8'] and 'head' in r['reason']
        elif m.in_channels <= 4:
            assert not r['int8'] and 'stem' in r['reason']
    int8 = {n for n, r in rows.items() if r['int8']}
    from models.encoders import resnet
    blocks = [n for n, m in mods.items() if isinstance(m, resnet.Bottleneck)]
    assert len(blocks) == 16 and {f'{b}.{c}' for b in blocks for c in ('conv1', 'conv2', 'conv3')} <= int8
    assert any('conv3_0' in n for n in int8) and any('conv3_1' in n for n in int8)
    assert len(int8) == len({id(r['conv']) for r in unet_state.rows})
    # depthwise convs stay 16-bit
    from models import unet
    from models.encoders import mobilenetv2
    mb = unet.UNet(2, mobilenetv2.mobilenet_v2(width_mult=0.35), 32, train_upsampling=True).eval()
    quant.prepare(mb)
    assert any(r['reason'] == 'depthwise' for r in quant.summary(mb))


def test_nothing_changes_outside_the_contexts(unet_state):
    st = unet_state
    assert torch.equal(st.before, st.after_convert) and torch.equal(st.before, st.after)


def test_state_round_trip(unet_state, hip_device):
    from ssseg import quant
    st = unet_state
    buf = io.BytesIO()
    torch.save({'state_dict': st.model.state_dict(), 'quant': quant.state_dict(st.model)}, buf)
    buf.seek(0)
    f = torch.load(buf, map_location='cpu')
    fresh = _build('unet', seed=5)
    fresh.load_state_dict(f['state_dict'])
    fresh = fresh.to(hip_device).eval()
    quant.load_state_dict(fresh, f['quant'], rule='all')
    y =_logits(quant.QuantizedModel(fresh)(st.x[2]))
    assert torch.equal(y, st.yq)
    # the derived int8 weights are dropped with the packed weights and re-derived from the masters
    from ssseg import nn as snn
    snn.invalidate_packed(fresh)
    assert all(rec.qw is None for rec in fresh.__dict__['_ssseg_quant_recs'])
    assert torch.equal(_logits(quant.QuantizedModel(fresh)(st.x[2])), st.yq)


def test_graph_capture_replays_bitwise(unet_state):
    from ssseg import quant
    st = unet_state
    qm = quant.QuantizedModel(st.model)
    buf = st.x[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qm(buf)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _logits(qm(buf))
    buf.copy_(st.x[2])                            # a new input
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, st.yq)


def test_wrappers_take_the_quantized_model(unet_state):
    from models.inference_wrapper import InferenceWrapper
    from ssseg import quant, sliding
    st = unet_state
    qm = quant.QuantizedModel(st.model)
    mask, prob = InferenceWrapper(qm)(st.x[2][0])
    assert tuple(mask.shape) == (2, 64, 64) and tuple(prob.shape) == (2, 64, 64)
    fused = sliding.SlidingWindowInference(qm, crop_size=64, stride=32, window_batch=2)(
        torch.rand(1, 3, 96, 64, device=st.x[0].device))
    assert tuple(fused.shape) == (1, 2, 96, 64) and fused.dtype == torch.float32
    assert bool(torch.isfinite(fused).all())


def test_quantized_refuses_an_input_that_requires_grad(unet_state):
    from ssseg import quant
    st = unet_state
    x = st.x[2].clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        quant.QuantizedModel(st.model)(x)
    with pytest.raises(RuntimeError):
        with quant.quantized(st.model, x):
            pass
    with torch.no_grad():                          # with autograd off the same tensor is an ordinary input
        assert torch.equal(_logits(quant.QuantizedModel(st.model)(x)), st.yq)


CFG = """
from functools import partial
import torch
import losses
from data.synthetic import SyntheticSegDataset
from models import simple_unet
from models.adapters import ListOutput
common = dict(world_size=1, use_cpu=False, workers=0, output_dir='runs/t', num_classes=3, image_size=32,
              compute_dtype='bf16')
model = dict(model_fn=lambda: ListOutput(simple_unet.UNet(3, num_blocks=2, first_channels=8, max_width=32)))
train = dict(unsupervised_dataset=partial(SyntheticSegDataset, length=6, size=32, seed=3, with_masks=False,
                                          blob_sigma=3.0))
val = dict(batch_size_per_worker=2, dataset=partial(SyntheticSegDataset, length=4, size=32, seed=2, num_classes=3,
                                                    label_map=True, blob_sigma=3.0))
"""


def test_inference_entry_point(tmp_path, hip_device):
    """inference.py on SyntheticSegDataset with 4 calibration images: the file and the JSON line"""
    from models import simple_unet
    from models.adapters import ListOutput
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(CFG)
    torch.manual_seed(0)
    net = ListOutput(simple_unet.UNet(3, num_blocks=2, first_channels=8, max_width=32))
    _randomize_bn(net, 3)
    ck = tmp_path / 'ck.pth'
    torch.save({'ema_state_dict': net.state_dict()}, ck)
    out = tmp_path / 'model_quantized.pth'
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get('PYTHONPATH', '')]))
    p = subprocess.run([sys.executable, os.path.join(PKG, 'inference.py'), str(cfg), '--checkpoint', str(ck), '--out',
                        str(out), '--calib-images', '4', '--batch-size', '2', '--rule', 'all'], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc['calibration_images'] == 4 and doc['convs_int8'] >= 1 and doc['rule'] == 'all'
    assert 0.0 <= doc['argmax_agreement'] <= 1.0
    assert 0.0 <= doc['miou_16bit'] <= 100.0 and 0.0 <= doc['miou_int8'] <= 100.0
    f = torch.load(out, map_location='cpu')
    assert set(f) == {'state_dict', 'quant', 'meta'} and len(f['quant']) == doc['convs_int8']
    assert set(f['state_dict']) == set(net.state_dict()) and f['meta']['argmax_agreement'] == doc['argmax_agreement']
