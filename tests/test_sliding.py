"""GPU: sliding-window, flip and multi-scale evaluation (ssseg/sliding.py, csrc/sliding.hip) against the host
restatement tests/sliding_ref.py.

Exact tests use stub models whose outputs are small integers: with uniform weights every partial sum is an integer
below 2^24, and a quotient of two such integers rounded once to fp32 is what the fp64 restatement gives after its cast
(a division carried out in 53 >= 2 * 24 + 2 bits and rounded again to 24 rounds like the direct one), so torch.equal
holds.  The toleranced tests take their bound from the restatement itself: its fp32 run's largest deviation from its
fp64 run on the same recorded model outputs is the yardstick, and the device may deviate 4 x that from the fp64 run
(it interpolates and sums in another association than torch).  Every such test prints its figures before it asserts.
"""
import pytest
import torch

import sliding_ref as R

pytestmark = pytest.mark.gpu


# ---- stub models -------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """records every input shape (and, with keep=True, every input)"""

    def __init__(self, keep=False):
        super().__init__()
        self.keep, self.shapes, self.inputs, self.modes = keep, [], [], []

    def forward(self, x):
        self.shapes.append(tuple(x.shape))
        self.modes.append((self.training, torch.is_grad_enabled()))
        if self.keep:
            self.inputs.append(x.detach().clone())
        return None, [self.logits(x)]


class Pointwise(Stub):
    """logits[c] = sum_k w[c, k] x[k] per pixel, at the crop's own resolution; elementwise products and a 3-term sum
    (no GEMM), exact on integer inputs.  pool: a 2 x average pool behind it (h = ch / 2).  poison: what a crop of
    zeros (a null window) returns."""

    def __init__(self, w, dev, pool=False, poison=None, keep=False):
        super().__init__(keep)
        self.w, self.pool, self.poison = w.float().to(dev), pool, poison

    def logits(self, x):
        y = (self.w.view(1, -1, 3, 1, 1) * x.float().unsqueeze(1)).sum(2)
        if self.pool:
            y = torch.nn.functional.avg_pool2d(y, 2)
        if self.poison is not None:
            y[x.abs().amax((1, 2, 3)) == 0] = self.poison
        return y


class Position(Stub):
    """ignores its input: lx + 64 ly + 4096 (index in batch) + 2^18 c"""

    def __init__(self, C):
        super().__init__()
        self.C = C

    def logits(self, x):
        n, _, ch, cw = x.shape
        f = lambda v, shape: torch.arange(v, device=x.device, dtype=torch.float32).view(shape)
        return (f(cw, (1, 1, 1, cw)) + 64 * f(ch, (1, 1, ch, 1)) + 4096 * f(n, (n, 1, 1, 1))
                + 2.0 ** 18 * f(self.C, (1, self.C, 1, 1))).contiguous()


class Recorder(torch.nn.Module):
    """wraps a model and keeps the last logit map of every forward, window by window, on the host"""

    def __init__(self, m):
        super().__init__()
        self.m, self.outputs = m, []

    def forward(self, x):
        f, maps = self.m(x)
        self.outputs += list(maps[-1].detach().float().cpu())
        return f, maps


def run(model, image, crop, dev, **kw):
    from ssseg import sliding
    s = sliding.SlidingWindowInference(model, crop, **kw)
    out = s(image.float().to(dev))
    torch.cuda.synchronize()
    return s, out.cpu()


def restate(rec_outputs, B, size, crop, stride, scales, flip, wb, activation, weighting, dtype=torch.float64):
    """the restatement on the recorded per-window outputs, cut per scale by the window counts"""
    per_scale, at = [], 0
    for s in scales:
        Hs, Ws = R.scaled_size(*size, s)
        table = R.rows(B, Hs, Ws, crop, stride, flip, wb)
        per_scale.append((rec_outputs[at:at + len(table)], table, (Hs, Ws)))
        at += len(table)
    assert at == len(rec_outputs)
    return R.fused_map(per_scale, B, size, crop, activation, weighting, dtype)


def n_windows(B, size, crop, stride, flip):
    return len(R.rows(B, *size, crop, stride, flip))


# ---- 1. exact, pointwise stub ------------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
@pytest.mark.parametrize('size,crop,stride,B,wb,C', [
    ((40, 72), (32, 32), 24, 1, 4, 19), ((40, 72), (32, 32), 24, 3, 'all', 2), ((37, 53), (32, 32), 24, 3, 4, 19),
    ((37, 53), (32, 64), 32, 1, 1, 64), ((20, 50), (32, 32), 24, 3, 4, 1), ((20, 50), (32, 64), 24, 1, 1, 2),
    ((32, 32), (32, 32), 24, 3, 4, 64), ((64, 64), (32, 32), 32, 1, 'all', 19), ((64, 64), (32, 64), 32, 3, 4, 1),
    ((40, 72), (32, 64), 32, 3, 1, 2)], ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pointwise_stub_is_exact(hip_device, size, crop, stride, B, wb, C, flip):
    H, W = size
    img, w = R.integer_image(B, H, W, seed=H * W + C), R.mix_weights(C, seed=C)
    nb = n_windows(B, size, crop, (stride, stride), flip) if wb == 'all' else wb
    stub = Pointwise(w, hip_device, keep=True)
    _, out = run(stub, img, crop, hip_device, stride=stride, flip=flip, activation='none', window_batch=nb)
    want = R.pointwise(img, w).float()
    assert out.shape == want.shape and out.dtype == torch.float32
    assert torch.equal(out, want)
    # an image smaller than the crop: the crops read zeros outside it
    crops = torch.cat(stub.inputs).cpu()
    real = n_windows(B, size, crop, (stride, stride), False)
    views = [crops[:real]] + ([crops[real:2 * real].flip(-1)] if flip else [])   # a mirrored crop, mirrored back
    for v in views:
        assert float(v[:, :, :min(H, crop[0]), :min(W, crop[1])].min()) >= 1
        if H < crop[0]:
            assert float(v[:, :, H:, :].abs().max()) == 0
        if W < crop[1]:
            assert float(v[:, :, :, W:].abs().max()) == 0
    assert stub.modes and all(m == (False, False) for m in stub.modes)        # eval mode, no_grad
    assert stub.training                                                     # and the model's mode is restored


# ---- 2. exact, position stub -------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,crop,stride,B,wb,flip', [
    ((40, 72), (32, 32), 24, 3, 4, False), ((40, 72), (32, 32), 24, 3, 'all', True), ((37, 53), (32, 64), 24, 1, 1, True),
    ((64, 64), (32, 32), 32, 3, 4, True), ((20, 50), (32, 32), 24, 1, 4, False)],
    ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_position_stub_matches_restatement_exactly(hip_device, size, crop, stride, B, wb, flip):
    from ssseg import sliding
    C = 2
    nb = n_windows(B, size, crop, (stride, stride), flip) if wb == 'all' else wb
    rec = Recorder(Position(C))
    img = torch.zeros(B, 3, *size)
    s, out = run(rec, img, crop, hip_device, stride=stride, flip=flip, activation='none', window_batch=nb)
    want, wsum = restate(rec.outputs, B, size, crop, (stride, stride), (1.0,), flip, nb, 'none', 'uniform')
    assert torch.equal(out, want.float())
    # the weight map, from the kernels themselves on the same recorded outputs
    table, host = sliding.window_table(s.windows(B, *size), hip_device)
    frame = (max(size[0], crop[0]), max(size[1], crop[1]))
    acc = torch.zeros(B, C, *frame, device=hip_device)
    ws = torch.zeros(B, *frame, device=hip_device)
    logits = torch.stack(rec.outputs).to(hip_device)
    for k in range(0, len(table), 64):
        sliding.window_accumulate(logits[k:k + 64], table[k:k + 64], host[k:k + 64], crop, acc, ws, 'none', 'uniform')
    assert torch.equal(ws.cpu(), wsum.float())
    assert torch.equal((acc / ws[:, None]).cpu()[:, :, :size[0], :size[1]], want.float())


# ---- 3. batch invariance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,crop,B,C,pool', [((40, 72), (32, 32), 3, 19, True), ((37, 53), (32, 64), 1, 64, False),
                                                ((64, 64), (32, 32), 3, 2, True)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_window_batch_does_not_change_a_bit(hip_device, size, crop, B, C, pool):
    g = torch.Generator().manual_seed(7)
    img = torch.rand(B, 3, *size, generator=g)
    w = torch.randn(C, 3, generator=g) * 2
    outs = []
    for wb in (1, 4, n_windows(B, size, crop, (24, 24), True)):
        stub = Pointwise(w, hip_device, pool=pool)
        outs.append(run(stub, img, crop, hip_device, stride=24, flip=True, activation='softmax',
                        weighting='gaussian', window_batch=wb)[1])
    assert torch.isfinite(outs[0]).all() and float(outs[0].std()) > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # and twice the same call gives the same bits
    again = run(Pointwise(w, hip_device, pool=pool), img, crop, hip_device, stride=24, flip=True, activation='softmax',
                weighting='gaussian', window_batch=4)[1]
    assert torch.equal(again, outs[1])


# ---- 4. one shape, null windows ----------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_one_input_shape_and_null_windows(hip_device, flip):
    size, crop, B, C, wb = (40, 72), (32, 32), 3, 4, 8
    img, w = R.integer_image(B, *size, seed=2), R.mix_weights(C, seed=1)
    real = n_windows(B, size, crop, (24, 24), flip)                    # 18 or 36: neither a multiple of 8
    stub = Pointwise(w, hip_device, keep=True)
    s, out = run(stub, img, crop, hip_device, stride=24, flip=flip, activation='none', window_batch=wb)
    assert set(stub.shapes) == {(wb, 3, 32, 32)} and len(stub.shapes) == -(-real // wb)
    crops = torch.cat(stub.inputs).cpu()
    assert float(crops[real:].abs().max()) == 0 and float(crops[:real].abs().amax((1, 2, 3)).min()) > 0
    # a model that returns 1e30 for the null crops changes nothing
    poisoned = Pointwise(w, hip_device, poison=1e30)
    _, out2 = run(poisoned, img, crop, hip_device, stride=24, flip=flip, activation='none', window_batch=wb)
    assert torch.equal(out2, out) and torch.equal(out, R.pointwise(img, w).float())
    # the tables of a shape are built once: a second call on it uploads nothing new
    tables = dict(s._tables)
    s(img.float().to(hip_device))
    assert s._tables.keys() == tables.keys() and all(s._tables[k][2] is tables[k][2] for k in tables)


# ---- 5. half-resolution output, activations, Gaussian weights, scales -------------------------------------------
def _check_against_restatement(tag, out, rec_outputs, B, size, crop, stride, scales, flip, wb, activation, weighting):
    ref, _ = restate(rec_outputs, B, size, crop, stride, scales, flip, wb, activation, weighting, torch.float64)
    f32, _ = restate(rec_outputs, B, size, crop, stride, scales, flip, wb, activation, weighting, torch.float32)
    yard = float((f32.double() - ref).abs().max())
    dev = float((out.double() - ref).abs().max())
    print(f'{tag}: fp32 restatement vs fp64 {yard:.3e}, device vs fp64 {dev:.3e}, ratio {dev / max(yard, 1e-300):.2f}, '
          f'|ref| max {float(ref.abs().max()):.3f}')
    assert dev <= 4 * yard


@pytest.mark.parametrize('activation,weighting,crop,C,B', [
    ('softmax', 'gaussian', (32, 32), 19, 3), ('softmax', 'uniform', (32, 64), 19, 1),
    ('sigmoid', 'gaussian', (32, 64), 19, 1), ('sigmoid', 'uniform', (32, 32), 2, 3),
    ('none', 'gaussian', (32, 32), 19, 1), ('none', 'uniform', (32, 32), 64, 1),
    ('softmax', 'gaussian', (32, 32), 2, 1), ('softmax', 'gaussian', (32, 64), 64, 1),
    ('sigmoid', 'gaussian', (32, 32), 1, 3)], ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_half_resolution_scales_against_restatement(hip_device, activation, weighting, crop, C, B):
    size, scales, wb, stride = (40, 72), (0.5, 1.0, 1.5), 4, (24, 24)
    g = torch.Generator().manual_seed(C + B)
    img = torch.rand(B, 3, *size, generator=g)
    w = (torch.rand(C, 3, generator=g) * 2 - 1) * 2.5                  # |logit| <= 7.5: no softmax saturation
    rec = Recorder(Pointwise(w, hip_device, pool=True))
    _, out = run(rec, img, crop, hip_device, stride=24, scales=scales, flip=True, activation=activation,
                 weighting=weighting, window_batch=wb)
    assert rec.outputs[0].shape == (C, crop[0] // 2, crop[1] // 2)
    assert float(torch.stack(rec.outputs).abs().max()) <= 8
    _check_against_restatement(f'{activation}/{weighting} crop {crop} C {C} B {B}', out, rec.outputs, B, size, crop,
                               stride, scales, True, wb, activation, weighting)


# ---- 6. predict --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,crop,B,C', [((40, 72), (32, 32), 3, 19), ((37, 53), (32, 64), 1, 64),
                                           ((64, 64), (32, 32), 1, 2)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_predict_is_the_argmax_of_the_whole_image_function(hip_device, size, crop, B, C):
    from ssseg import sliding
    img, w = R.tiefree_image(B, *size, seed=C), R.mix_weights(C, seed=C + 1)
    full = R.pointwise(img, w)
    top2 = full.topk(min(2, C), dim=1).values
    assert C == 1 or float((top2[:, 0] - top2[:, 1]).min()) > 0         # no ties, by construction
    s = sliding.SlidingWindowInference(Pointwise(w, hip_device), crop, stride=24, flip=True, activation='none',
                                       window_batch=4)
    labels = s.predict(img.float().to(hip_device))
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (B, *size)
    assert torch.equal(labels.cpu(), full.argmax(1))


# ---- 7. argument errors ------------------------------------------------------------------------------------------
def test_argument_errors(hip_device):
    from ssseg import sliding
    dev = hip_device

    def accumulate(n, C, rows, frame=(8, 8), crop=(4, 4)):
        table, host = sliding.window_table(rows, dev)
        sliding.window_accumulate(torch.zeros(n, C, 4, 4, device=dev), table, host, crop,
                                  torch.zeros(1, C, *frame, device=dev), torch.zeros(1, *frame, device=dev), 'none')

    accumulate(64, 64, [(0, 4, 4, 0)] * 64)                             # the limits themselves pass
    with pytest.raises(RuntimeError, match='SSSEG_EINVAL'):
        accumulate(1, 65, [(0, 0, 0, 0)])
    with pytest.raises(RuntimeError, match='SSSEG_EINVAL'):
        accumulate(65, 1, [(0, 0, 0, 0)] * 65)
    for row in [(0, 5, 0, 0), (0, 0, 5, 0), (0, -1, 0, 0), (0, 0, -1, 1), (1, 0, 0, 0), (-1, 0, 0, 0)]:
        with pytest.raises(RuntimeError, match='SSSEG_EINVAL'):
            accumulate(2, 3, [(0, 0, 0, 0), row])
    accumulate(2, 3, [(0, 0, 0, 0), (7, 99, -5, sliding.NULL)])         # a null window's fields are not looked at
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        sliding.SlidingWindowInference(Pointwise(R.mix_weights(2), dev), 32)(torch.zeros(1, 3, 40, 72))
    table, host = sliding.window_table([(0, 0, 0, 0)], dev)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        sliding.window_gather(torch.zeros(1, 3, 8, 8), table, (4, 4))
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        sliding.window_accumulate(torch.zeros(1, 2, 4, 4), table, host, (4, 4), torch.zeros(1, 2, 8, 8, device=dev),
                                  torch.zeros(1, 8, 8, device=dev))
    with pytest.raises(ValueError):
        sliding.SlidingWindowInference(Pointwise(R.mix_weights(2), dev), 32, activation='tanh')


def test_gather_16_bit_and_strided_output(hip_device):
    """the gather moves 16-bit elements as they are and writes any layout: channels-last crops here"""
    from ssseg import sliding
    img = R.integer_image(2, 20, 50, seed=9).to(torch.bfloat16)
    rows = [(1, 0, 24, 0), (0, 0, 18, sliding.MIRROR), (0, 0, 0, sliding.NULL), (1, -3, 40, sliding.MIRROR)]
    table, _ = sliding.window_table(rows, hip_device)
    out = torch.empty(4, 3, 32, 32, dtype=torch.bfloat16, device=hip_device).contiguous(
        memory_format=torch.channels_last)
    got = sliding.window_gather(img.to(hip_device), table, (32, 32), out=out)
    assert got is out and out.is_contiguous(memory_format=torch.channels_last)
    padded = torch.zeros(2, 3, 80, 120, dtype=torch.bfloat16)
    padded[:, :, 10:30, 10:60] = img
    for j, (b, y0, x0, f) in enumerate(rows):
        want = padded[b, :, 10 + y0:42 + y0, 10 + x0:42 + x0]
        want = torch.zeros_like(want) if f & sliding.NULL else want.flip(-1) if f & sliding.MIRROR else want
        assert torch.equal(out[j].cpu(), want), j


# ---- 8. validate -------------------------------------------------------------------------------------------------
def test_validate_takes_the_fused_map(hip_device):
    import losses as L
    import train
    C, size = 4, (40, 72)
    # the signs of channels 2 and 1 of the tie-free image pick the winning row: every class wins about a quarter
    img, w = R.tiefree_image(2, *size, seed=5), torch.tensor([[1., 3, 3], [-1, -3, 3], [2, 3, -3], [-2, -3, -3]]).double()
    g = torch.Generator().manual_seed(11)
    labels = torch.randint(0, C, (2, *size), generator=g)
    labels[torch.rand(2, *size, generator=g) < 0.1] = 255
    # half of the valid pixels carry the model's own label, so the IoUs are neither 0 nor 100
    pred = R.pointwise(img, w).argmax(1)
    own = (torch.rand(2, *size, generator=g) < 0.5) & (labels != 255)
    labels[own] = pred[own]
    loader = [{'image': img[b:b + 1].float(), 'semantic_mask': labels[b:b + 1].to(torch.uint8)} for b in range(2)]
    loss = L.CalculateLoss([{'loss_fn': L.CrossEntropyLossWithLogits(ignore_index=255), 'weight': [1.0]}])
    cfg = {'train': {'loss': loss, 'ignore_label': 255},
           'val': {'sliding_window': dict(crop_size=32, stride=24, scales=(1.0,), flip=True, weighting='uniform',
                                          window_batch=4)}}
    stub = Pointwise(w, hip_device)
    val_loss, _ = train.validate(stub, loader, 0, 0, None, cfg, hip_device)
    valid = labels != 255
    ious = []
    for c in range(C):
        inter = int(((pred == c) & (labels == c) & valid).sum())
        union = int((((pred == c) | (labels == c)) & valid).sum())
        ious.append(100.0 * inter / union if union else 100.0)
    print('validate (sliding): class IoUs', train._VALIDATE['class_ious'], 'host', ious)
    assert set(stub.shapes) == {(4, 3, 32, 32)}
    assert train._VALIDATE['class_ious'] == pytest.approx(ious, rel=1e-9)
    assert train._VALIDATE['miou'] == pytest.approx(sum(ious) / C, rel=1e-9)
    assert 0 < min(ious) and max(ious) < 100
    # the loss saw the fused logits: cross-entropy of the whole-image function over the valid pixels
    ce = torch.nn.functional.cross_entropy(R.pointwise(img, w), labels, ignore_index=255, reduction='none')
    per_image = [float(ce[b][valid[b]].mean()) for b in range(2)]
    assert float(val_loss) == pytest.approx(sum(per_image) / 2, rel=1e-5)
    assert stub.training                                               # validate() leaves the model in train mode
    # without the key: the whole image in one forward, as before
    old = Pointwise(w, hip_device)
    train.validate(old, loader, 0, 0, None, {'train': cfg['train']}, hip_device)
    assert old.shapes == [(1, 3, 40, 72)] * 2
    assert train._VALIDATE['class_ious'] == pytest.approx(ious, rel=1e-9)


# ---- a real model --------------------------------------------------------------------------------------------------
def test_simple_unet_windows_against_restatement(hip_device):
    """SimpleUNet in the default 16-bit NHWC compute mode at crop 64 on a 96 x 160 image: the fused map is the
    restatement's on the recorded per-window logits, under the bound of the half-resolution test."""
    from models import simple_unet
    from models.adapters import ListOutput
    torch.manual_seed(0)
    C, size, crop = 5, (96, 160), (64, 64)
    net = ListOutput(simple_unet.UNet(C, 2, 8, 16))
    rec = Recorder(net.to(hip_device))
    img = torch.rand(2, 3, *size, generator=torch.Generator().manual_seed(4))
    s, out = run(rec, img, crop, hip_device, flip=True, activation='softmax', weighting='gaussian', window_batch=4)
    assert s.stride == (43, 43) and len(rec.outputs) == 2 * 2 * 4 * 2 and rec.outputs[0].shape[0] == C
    assert float(torch.stack(rec.outputs).abs().max()) <= 8 and float(torch.stack(rec.outputs).std()) > 0
    _check_against_restatement('SimpleUNet', out, rec.outputs, 2, size, crop, s.stride, (1.0,), True, 4, 'softmax',
                               'gaussian')
