"""Post-training int8 inference -- the deployment step of the reference's inference.py (torch.quantization
prepare / convert on fbgemm) on the integer MFMA pipe (csrc/quant.hip).

    quant.prepare(model)                       # mark the eligible convs, one device slot each
    with quant.calibrating(model):             # eval forwards: every eligible conv observes max |input|
        for images in loader: model(images)
    quant.convert(model, rule='all')           # int8 weights, frozen BN folds ('measured': only where int8 is faster)
    qmodel = quant.QuantizedModel(model)       # forward runs quantise + int8 conv for the converted convs
    torch.save({'state_dict': model.state_dict(), 'quant': quant.state_dict(model)}, path)

The scheme (include/ssseg.h, DESIGN.md "Post-training int8 inference"): symmetric int8 per-tensor activations at each
conv's input, symmetric int8 per-output-channel weights, exact int32 accumulation, and the 16-bit engine's folded
eval-BN / bias / residual / activation epilogue in fp32.  Outputs stay in the compute dtype, so the stem, the head,
ConvTranspose2d and depthwise convs run the existing path next to the int8 ones (mixed precision).  Every scale is a
device value: calibration and inference never synchronise, and a quantised forward captures into a HIP graph once one
eager forward has derived the int8 weights and folds.  Inference only: the contexts run under torch.no_grad().
"""
import contextlib
import ctypes

import torch
import torch.nn as nn

from . import native as N
from . import nn as snn

# convert() leaves a class of layers in the 16-bit path where its int8 form, quantise pass included, measured slower.
# The rule is static, on (R*S*Cin, Cout), chosen from tools/quant_ab.py's table (profiles/quant_ab.jsonl):
# (lowest contraction, highest contraction, lowest Cout, highest Cout) boxes in which int8 measured FASTER.  At the C2
# eval shapes no class did -- int8 / bf16 device time is 1.20 .. 2.44 over contractions 64 .. 10368 and Cout 64 .. 2048,
# 1.60 for the whole forward -- so the measured rule is empty, and rule='all' is how the int8 path is run today.
MEASURED_FASTER = ()
RULES = ('measured', 'all')


def worth_int8(contraction, cout, rule='measured'):
    """the static eligibility rule on (R*S*Cin, Cout)"""
    if rule not in RULES:
        raise ValueError(f'ssseg.quant: rule must be one of {RULES}, got {rule!r}')
    if rule == 'all':
        return True
    return any(k0 <= contraction <= k1 and c0 <= cout <= c1 for k0, k1, c0, c1 in MEASURED_FASTER)


class _Rec:
    """Per-conv quantisation record (conv.__dict__['_ssseg_q'])."""
    __slots__ = ('name', 'conv', 'slot', 'seen', 'converted', 'qw', 'sw', 'folds', 'why')

    def __init__(self, name, conv, slot):
        self.name, self.conv, self.slot = name, conv, slot
        self.seen = False        # reached by a calibration forward (or loaded from a state)
        self.converted = False
        self.why = None          # why convert() left it in the 16-bit path
        self.qw = self.sw = None
        self.folds = {}          # id(bn) or None -> (bn, scale, shift)

    def drop(self):
        """the parameters changed: the int8 weights and the folds are re-derived by the next quantised forward"""
        self.qw = self.sw = None
        self.folds = {}


def _static_reason(m):
    """why a module never runs int8 (None: eligible)"""
    if isinstance(m, snn.ConvTranspose2d):
        return 'ConvTranspose2d'
    if not isinstance(m, snn.Conv2d):
        return None
    if m._ssseg_dw:
        return 'depthwise'
    if m.groups != 1:
        return 'grouped'
    if m._ssseg_head:
        return 'head (fp32 logits)'
    if m.in_channels <= 4:
        return 'stem (Cin <= 4)'
    if max(m.kernel_size) > 7 or max(m.stride) > 2:
        return 'geometry (taps > 7 or stride > 2)'
    return None


def _recs(model):
    recs = model.__dict__.get('_ssseg_quant_recs')
    if recs is None:
        raise RuntimeError('ssseg.quant: call prepare(model) first')
    return recs


def prepare(model):
    """Mark the eligible convs of `model` (ssseg.nn.Conv2d, groups == 1, not a head, real Cin > 4) and give each a
    one-float device slot for its input's running max |x|.  Idempotent; returns the model."""
    if '_ssseg_quant_recs' in model.__dict__:
        return model
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, snn.Conv2d) and _static_reason(m) is None]
    dev = convs[0][1].weight.device if convs else torch.device('cpu')
    slots = torch.zeros(max(len(convs), 1), dtype=torch.float32, device=dev)
    recs = []
    for i, (name, m) in enumerate(convs):
        rec = _Rec(name, m, slots[i:i + 1])
        m.__dict__['_ssseg_q'] = rec
        recs.append(rec)
    model.__dict__['_ssseg_quant_recs'] = recs
    model.__dict__['_ssseg_quant_slots'] = slots
    return model


# ---- trace ---------------------------------------------------------------------------------------------------------
_TRACE = [None]


@contextlib.contextmanager
def trace():
    """Diagnostic: keeps a reference to every observed / quantised launch inside the block.  Yields a list of dicts
    {'mode': 'calibrate' | 'int8', 'conv', 'input', 'q' (int8 [N,H,W,rup(Cin,16)] or None), 'residual', 'output',
    'bn', 'act'}."""
    rows = []
    prev, _TRACE[0] = _TRACE[0], rows
    try:
        yield rows
    finally:
        _TRACE[0] = prev


# ---- the per-conv hooks (ssseg.nn.Conv2d._ssseg_forward) -----------------------------------------------------------
def _observe(conv, x, relu, bn, residual):
    rec = conv.__dict__.get('_ssseg_q')
    if rec is None:
        return None
    snn.materialize(x)
    n, cp, H, W = x.shape
    N.call('ssseg_absmax_update', N.dev_ptr(x), n * H * W, conv.in_channels, cp, N.dt_code(x), N.dev_ptr(rec.slot),
           N.stream())
    rec.seen = True
    if _TRACE[0] is not None:
        _TRACE[0].append({'mode': 'calibrate', 'conv': conv, 'input': x, 'q': None, 'residual': residual,
                          'output': None, 'bn': bn, 'act': relu})
    return None   # the unchanged 16-bit path runs the layer


def _derive_weights(rec):
    conv = rec.conv
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('ssseg.quant: the int8 weights are not derived yet (or were dropped by invalidate_packed); '
                           'run one eager quantised forward before capturing a graph')
    K, C, R, S = conv.weight.shape
    Kp, Cq = snn.rup(conv._dims()[1], 16), snn.rup(C, 16)
    w = conv.weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    if w.dtype != torch.float32:
        raise RuntimeError('ssseg.quant: fp32 master weights expected')
    rec.qw = torch.empty(Kp * R * S * Cq, dtype=torch.int8, device=w.device)
    rec.sw = torch.empty(Kp, dtype=torch.float32, device=w.device)
    N.call('ssseg_weight_quant_i8', N.dev_ptr(w, 'weight'), K, C, R, S, Kp, Cq, N.dev_ptr(rec.qw), N.dev_ptr(rec.sw),
           N.stream())


def _derive_fold(rec, bn):
    """(scale, shift) of the epilogue, frozen: the eval BN (+ conv bias) folded once by ssseg_bn_fold, or the bias"""
    conv = rec.conv
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('ssseg.quant: a BN fold is not derived yet; run one eager quantised forward before '
                           'capturing a graph')
    cout = conv._dims()[1]
    dev = conv.weight.device
    if bn is None:
        shift = None
        if conv.bias is not None:
            shift = torch.zeros(cout, dtype=torch.float32, device=dev)
            shift[:conv.out_channels] = conv.bias.detach().float()
        fold = (None, None, shift)
    else:
        if bn.training or not bn.track_running_stats:
            raise RuntimeError('ssseg.quant: the int8 path folds eval-mode BatchNorm only; call model.eval()')
        if bn.num_features != conv.out_channels:
            raise ValueError('ssseg.quant: BatchNorm width != conv out_channels')
        v = torch.empty(2 * cout, dtype=torch.float32, device=dev)
        opt = lambda t: N.dev_ptr(t.detach()) if t is not None else None  # noqa: E731
        N.call('ssseg_bn_fold', N.dev_ptr(bn.running_mean), N.dev_ptr(bn.running_var), opt(bn.weight), opt(bn.bias),
               opt(conv.bias), float(bn.eps), bn.num_features, cout, N.dev_ptr(v[:cout]), N.dev_ptr(v[cout:]), None,
               None, N.stream())
        fold = (bn, v[:cout], v[cout:])
    rec.folds[id(bn) if bn is not None else None] = fold
    return fold


def _int8(conv, x, relu, bn, residual):
    rec = conv.__dict__.get('_ssseg_q')
    if rec is None or not rec.converted:
        return None
    if rec.qw is None:
        _derive_weights(rec)
    fold = rec.folds.get(id(bn) if bn is not None else None)
    if fold is None or fold[0] is not bn:
        fold = _derive_fold(rec, bn)
    _, scale, shift = fold
    snn.materialize(x)
    n, cp, H, W = x.shape
    cout = conv._dims()[1]
    C = conv.in_channels
    ldq = snn.rup(C, 16)
    q = torch.empty((n, H, W, ldq), dtype=torch.int8, device=x.device)
    N.call('ssseg_quantize_i8', N.dev_ptr(x), n * H * W, C, cp, N.dt_code(x), N.dev_ptr(rec.slot), N.dev_ptr(q), ldq,
           N.stream())
    d = conv._fwd_desc(n, H, W)
    R, S = conv.kernel_size
    d.C, d.ldx, d.ldw = ldq, ldq, R * S * ldq
    y = snn.new_act(n, cout, d.OH, d.OW, x.dtype, x.device)
    snn._need_res(residual, y)
    code, slope = snn._act(relu)
    ep = N.ConvEpilogue(N.dev_ptr(scale) if scale is not None else None,
                        N.dev_ptr(shift) if shift is not None else None,
                        N.dev_ptr(residual) if residual is not None else None,
                        residual.shape[1] if residual is not None else 0, None, code, slope)
    N.call('ssseg_conv_i8_fwd', N.dev_ptr(q), N.dev_ptr(rec.qw), N.dev_ptr(y), ctypes.byref(d), N.dt_code(y),
           N.dev_ptr(rec.slot), N.dev_ptr(rec.sw), ctypes.byref(ep), N.stream())
    if _TRACE[0] is not None:
        _TRACE[0].append({'mode': 'int8', 'conv': conv, 'input': x, 'q': q, 'residual': residual, 'output': y,
                          'bn': bn, 'act': relu, 'scale': scale, 'shift': shift})
    return y


@contextlib.contextmanager
def _hooked(hook):
    prev, snn._QUANT[0] = snn._QUANT[0], hook
    try:
        with torch.no_grad():
            yield
    finally:
        snn._QUANT[0] = prev


def calibrating(model):
    """Context: every eligible conv's forward first folds max |input| (finite values, real channels) into its slot,
    then runs the unchanged 16-bit path.  A conv called several times per forward shares one slot."""
    _recs(model)
    if model.training:
        raise RuntimeError('ssseg.quant.calibrating: eval mode expected (model.eval())')
    return _hooked(_observe)


def convert(model, rule='measured'):
    """Quantise and pack the weights of every calibrated conv and freeze its BN fold (pairs seen in calibration; others
    fold at their first quantised forward).  rule='measured' (default) leaves the layer classes that measured slower in
    int8 in the 16-bit path (worth_int8); rule='all' converts every calibrated eligible conv.  Requires eval mode.
    Returns the model."""
    recs = _recs(model)
    if model.training:
        raise RuntimeError('ssseg.quant.convert: eval mode expected (model.eval())')
    worth_int8(0, 0, rule)
    for rec in recs:
        conv = rec.conv
        R, S = conv.kernel_size
        rec.drop()
        if not rec.seen:
            rec.converted, rec.why = False, 'not reached by a calibration forward'
        elif not worth_int8(R * S * conv.in_channels, conv.out_channels, rule):
            rec.converted, rec.why = False, 'slower in int8 (measured rule on R*S*Cin, Cout)'
        else:
            rec.converted, rec.why = True, None
            if conv.weight.is_cuda:
                _derive_weights(rec)
    return model


def quantized(model, *inputs):
    """Context: the converted convs run ssseg_quantize_i8 + ssseg_conv_i8_fwd.  Inference only: an input that requires
    grad while autograd is enabled is an error."""
    _recs(model)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
        raise RuntimeError('ssseg.quant.quantized: the int8 path is inference only (input requires grad)')
    if model.training:
        raise RuntimeError('ssseg.quant.quantized: eval mode expected (model.eval())')
    return _hooked(_int8)


class QuantizedModel(nn.Module):
    """nn.Module whose forward runs `model` inside quantized(model): InferenceWrapper, SlidingWindowInference and the
    pool scorer take it in place of the model."""

    def __init__(self, model):
        super().__init__()
        _recs(model)
        self.model = model
        self.eval()

    def forward(self, *args, **kw):
        with quantized(self.model, *args, *kw.values()):
            return self.model(*args, **kw)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__('model'), name)


def state_dict(model):
    """{qualified conv name: slot value (0-d fp32 CPU tensor)} of the calibrated convs.  The int8 weights are
    re-derived from the master weights."""
    return {rec.name: rec.slot.detach().cpu().reshape(()).clone() for rec in _recs(model) if rec.seen}


def load_state_dict(model, state, rule='measured'):
    """Restore calibrated slots into `model` (prepared here if needed) and convert it under `rule`."""
    prepare(model)
    recs = {rec.name: rec for rec in _recs(model)}
    unknown = sorted(set(state) - set(recs))
    if unknown:
        raise KeyError(f'ssseg.quant.load_state_dict: no eligible conv named {unknown[:3]}')
    for rec in recs.values():
        rec.seen = rec.name in state
        rec.slot.fill_(float(state[rec.name]) if rec.seen else 0.0)
    return convert(model, rule)


def summary(model):
    """[{'name', 'int8': bool, 'reason': why not (None for int8)}] for every conv of the model."""
    recs = model.__dict__.get('_ssseg_quant_recs')
    rows = []
    for name, m in model.named_modules():
        if not isinstance(m, (snn.Conv2d, snn.ConvTranspose2d)):
            continue
        rec = m.__dict__.get('_ssseg_q')
        why = _static_reason(m)
        if why is None:
            if recs is None or rec is None:
                why = 'not prepared'
            elif not rec.converted:
                why = rec.why or ('not converted' if rec.seen else 'not calibrated')
        rows.append({'name': name, 'int8': why is None, 'reason': why})
    return rows
