"""Host-side checks (no GPU) of the losses beyond BCE / Lovász / RMI.

The CPU yardstick of these losses lives here: a plain-PyTorch fp64 restatement of each formula (reference
losses.py:25-268).  It must reproduce every golden loss and gradient that tests/golden/gen_golden_losses.py recorded
from the reference in fp32, which pins the fixtures and the yardstick to each other; the GPU tests
(test_hip_losses_ext.py) import both from here.  Also: constructor behaviour and host-side argument validation of
the new C ABI.
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

F64 = torch.float64


# ---- fp64 restatements -------------------------------------------------------------------------------------------
def ce64(x, t, reduction='mean'):
    l = -(t * torch.log_softmax(x, 1)).sum(1)
    return l.mean() if reduction == 'mean' else l


def ohem_state64(x, t, thres, min_kept):
    """(threshold, selection mask [B,H,W]) of OhemCrossEntropy"""
    pred = torch.softmax(x, 1).gather(1, t.argmax(1, keepdim=True)).squeeze(1)
    flat = pred.reshape(-1).sort()[0]
    thr = max(float(flat[min(max(1, min_kept), flat.numel() - 1)]), thres)
    return thr, pred < thr


def ohem64(x, t, thres, min_kept):
    _, sel = ohem_state64(x.detach(), t, thres, min_kept)
    return ce64(x, t, 'none')[sel].mean()


def focal64(x, t, alpha, gamma):
    ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    p = torch.sigmoid(x)
    pt = t * p + (1 - t) * (1 - p)
    return ((1 - pt) ** gamma * (t * alpha + (1 - t) * (1 - alpha)) * ce).mean()


def nfl64(x, lab, k_sum, alpha=0.25, gamma=2, from_logits=False, weight=1.0, size_average=True, eps=1e-12,
          scale=1.0, ignore_label=-1, **_):
    """-> (loss [B], new k_sum)"""
    pred = x if from_logits else torch.sigmoid(x)
    pos, valid = lab > 0, lab != ignore_label
    al = torch.where(pos, torch.tensor(alpha, dtype=x.dtype), torch.tensor(1 - alpha, dtype=x.dtype))
    pt = torch.where(valid, torch.where(pos, pred, 1 - pred), torch.ones_like(pred))
    beta = (1 - pt) ** gamma
    hw = float(lab.shape[-2] * lab.shape[-1])
    mult = (hw / (beta.sum((-2, -1), keepdim=True) + eps)).detach()
    clean = (lab == -1).flatten(1).sum(1) == 0
    if bool(clean.any()):
        k_sum = 0.9 * k_sum + 0.1 * float(mult.flatten(1).mean(1)[clean].mean())
    loss = weight * (-al * beta * mult * torch.log(torch.clamp(pt + eps, max=1.0)) * valid)
    loss = loss.flatten(1).sum(1)
    if size_average:
        loss = loss / (valid.flatten(1).sum(1) + eps)
    return scale * loss, k_sum


def dice_logits64(x, t):
    p = torch.softmax(x, 1)
    mask = (t.sum((2, 3)) > 1.).to(x.dtype)
    dice = (2. * (p * t).sum((2, 3)) + 1.) / ((p + t).sum((2, 3)) + 1.)
    return 1 - ((dice * mask).sum(1) / mask.sum(1)).mean()


def dice_prob64(p, t, log_mode=False, gamma=1.0):
    r = (2. * (p * t).sum((1, 2, 3)) + 1.) / ((p + t).sum((1, 2, 3)) + 1.)
    return (-torch.log(r)) ** gamma if log_mode else 1 - r


def binary_entropy64(x):
    p = torch.sigmoid(x)
    # the one fp32 property the reference's result depends on: its sigmoid is exactly 1 for a large logit, and the
    # loss (and that element's gradient) NaN from 0 * log(0).  p / p is that exact 1 with the graph kept.
    p = torch.where(torch.sigmoid(x.detach().float()) == 1, p / p, p)
    return -(p * torch.log(p) + (1. - p) * torch.log(1. - p)).mean() / 2


def entropy64(x):
    return -(torch.softmax(x, 1) * torch.log_softmax(x, 1)).sum(1).mean()


def bce64(x, t, reduction):
    l = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return {'none': l, 'sum': l.sum(), 'mean': l.mean()}[reduction]


def smooth64(t, alpha):
    return t * (1 - alpha) + alpha / t.size(1)


# ---- the fixtures ------------------------------------------------------------------------------------------------
def nfl_kwargs(g):
    kw = {k[2:]: g[k].item() for k in g.files if k.startswith('p_')}
    kw.pop('axis', None)
    return kw


def _case(name):
    """name -> (callable on (x, t) in any dtype, kind)"""
    g = golden(f'losses_ext_{name}.npz')
    if name.startswith('ce_'):
        return lambda x, t: ce64(x, t, name.split('_')[1])
    if name.startswith('ohem_'):
        return lambda x, t: ohem64(x, t, float(g['thres']), int(g['min_kept']))
    if name.startswith('focal_'):
        return lambda x, t: focal64(x, t, float(g['alpha']), float(g['gamma']))
    if name.startswith('dice_'):
        return dice_logits64
    if name.startswith('nfl_'):
        return lambda x, t: nfl64(x, t, 0.0, **nfl_kwargs(g))[0]
    if name == 'dicep_s1':
        return dice_prob64
    if name.startswith('logdicep_'):
        return lambda p, t: dice_prob64(p, t, True, float(g['gamma']))
    if name.startswith('bent_'):
        return lambda x, t: binary_entropy64(x)
    if name.startswith('ent_'):
        return lambda x, t: entropy64(x)
    if name.startswith('bce_'):
        return lambda x, t: bce64(x, t, name.split('_')[1])
    raise KeyError(name)


CASES = sorted(os.path.basename(p)[len('losses_ext_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'losses_ext_*.npz'))
               if not p.endswith('smooth_s2.npz'))
NAN_CASES = ('dice_nan', 'bent_nan')
_REF64 = {}


def ref64(name):
    """fp64 loss and d (loss * w).sum() / d x of a fixture, computed once and shared (read-only)"""
    if name not in _REF64:
        g = golden(f'losses_ext_{name}.npz')
        x = torch.from_numpy(g['x']).to(F64).requires_grad_(True)
        t = torch.from_numpy(g['t']).to(F64) if 't' in g.files else None
        loss = _case(name)(x, t)
        (loss * torch.from_numpy(g['w']).to(F64)).sum().backward()
        _REF64[name] = (loss.detach().numpy(), x.grad.numpy())
    return _REF64[name]


def err(a, ref):
    """max |a - ref| over the finite entries of ref; the non-finite entries must match exactly in place"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), 'NaN pattern differs'
    assert np.array_equal(a[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    return float(np.abs(a[fin] - ref[fin]).max()) if fin.any() else 0.0


def test_fixture_set_is_complete():
    want = {'ce_mean_s1', 'ce_mean_s2', 'ce_mean_s3', 'ce_mean_soft', 'ce_none_s1', 'ohem_k100', 'ohem_k1000',
            'ohem_k5000', 'focal_s1', 'focal_s2', 'focal_s3', 'focal_soft', 'focal_g15', 'focal_sat', 'dice_s1',
            'dice_s2', 'dice_s3', 'dice_absent', 'dice_nan', 'nfl_default', 'nfl_s2', 'nfl_logits', 'nfl_sum',
            'dicep_s1', 'logdicep_s1', 'logdicep_g2', 'bent_in', 'bent_nan', 'ent_s1', 'ent_s2', 'ent_s3',
            'bce_none_s1', 'bce_sum_s1'}
    assert set(CASES) == want
    for p in glob.glob(os.path.join(GOLDEN, 'losses_ext_*.npz')):
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize('name', CASES)
def test_fp64_restatement_reproduces_golden(name):
    """The reference ran in fp32; the restatement runs in fp64.  Bound: the project's loss / gradient bounds
    (tests/test_hip_losses.py: loss rtol 2e-5 atol 1e-7, gradient rtol 2e-4 atol 2e-8), the gradient's relative part
    taken against the largest gradient entry: an entry that cancels to ~0 carries the absolute rounding error of its
    terms, which scales with the large entries, not with itself."""
    g = golden(f'losses_ext_{name}.npz')
    loss, grad = ref64(name)
    assert g['loss'].shape == loss.shape and g['grad'].shape == grad.shape
    if name in NAN_CASES:
        assert np.isnan(g['loss']).all() and np.isnan(loss).all()
    else:
        assert np.isfinite(g['loss']).all()
        el = err(g['loss'], loss)
        print(f'{name}: loss err {el:.3e}')
        assert el <= 2e-5 * float(np.abs(loss).max()) + 1e-7
    eg = err(g['grad'], grad)
    gmax = float(np.abs(grad[np.isfinite(grad)]).max())
    print(f'{name}: grad err {eg:.3e} (max |grad| {gmax:.3e})')
    assert gmax > 0 and eg <= 2e-4 * gmax + 2e-8


def test_ohem_regimes():
    for min_kept, kept in ((100, 928), (1000, 1000), (5000, 1151)):
        g = golden(f'losses_ext_ohem_k{min_kept}.npz')
        assert int(g['kept']) == kept
        x, t = torch.from_numpy(g['x']).to(F64), torch.from_numpy(g['t']).to(F64)
        thr, sel = ohem_state64(x, t, float(g['thres']), min_kept)
        assert int(sel.sum()) == kept and abs(thr - float(g['threshold'])) < 1e-6


def test_nfl_k_sum_and_second_call():
    for name in ('nfl_default', 'nfl_s2', 'nfl_logits', 'nfl_sum'):
        g = golden(f'losses_ext_{name}.npz')
        k, ks = 0.0, []
        for xk, tk in (('x', 't'), ('x2', 't2')):
            loss, k = nfl64(torch.from_numpy(g[xk]).to(F64), torch.from_numpy(g[tk]).to(F64), k, **nfl_kwargs(g))
            ks.append(k)
        np.testing.assert_allclose(ks, g['k_sum'], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(loss.numpy(), g['loss2'], rtol=2e-5, atol=1e-7)
    assert list(golden('losses_ext_nfl_logits.npz')['k_sum']) == [0.0, 0.0]   # every sample has a -1 label
    assert golden('losses_ext_nfl_default.npz')['k_sum'][0] > 0


def test_smooth_labels_fixture():
    g = golden('losses_ext_smooth_s2.npz')
    np.testing.assert_allclose(smooth64(torch.from_numpy(g['t']).to(F64), float(g['alpha'])).numpy(), g['out'],
                               rtol=1e-6, atol=0)


# ---- constructors ------------------------------------------------------------------------------------------------
def test_constructor_defaults_equal_the_reference():
    import losses as L
    m = L.OhemCrossEntropy()
    assert (m.thresh, m.min_kept) == (0.7, 100000) and L.OhemCrossEntropy(min_kept=0).min_kept == 1
    assert m.criterion.reduction == 'none'
    m = L.FocalLoss()
    assert (m.alpha, m.gamma) == (0.25, 2.0)
    m = L.NormalizedFocalLossSigmoid()
    assert (m._axis, m._alpha, m._gamma, m._from_logits, m._batch_axis, m._weight, m._size_average,
            m._detach_delimeter, m._eps, m._scale, m._ignore_label, m._k_sum) == (
        -1, 0.25, 2, False, 0, 1.0, True, True, 1e-12, 1.0, -1, 0)
    assert L.DenseCrossEntropyLossWithLogits().reduction == 'mean'
    assert L.DenseBinaryCrossEntropyLossWithLogits().reduction == 'mean'
    assert L.DenseBinaryCrossEntropyLossWithLogits('sum').reduction == 'sum'
    L.DiceWithLogitsLoss()
    assert L.get_dims_with_exclusion(4, 0) == [1, 2, 3] and L.get_dims_with_exclusion(3) == [0, 1, 2]
    for n in ('dice_loss', 'log_dice_loss', 'binary_entropy_loss', 'entropy_loss', 'smooth_labels'):
        assert callable(getattr(L, n))


def test_constructor_refusals():
    import losses as L
    with pytest.raises(NotImplementedError):
        L.NormalizedFocalLossSigmoid(detach_delimeter=False)
    with pytest.raises(NotImplementedError):
        L.NormalizedFocalLossSigmoid(weight=torch.ones(2))
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match='incorrect value of reduction'):   # as the reference: at the call
        L.DenseCrossEntropyLossWithLogits('sum')(x, x)
    with pytest.raises(RuntimeError, match='HIP device tensor'):            # and no CPU fallback
        L.FocalLoss()(x, x)


# ---- the C ABI validates on the host -----------------------------------------------------------------------------
def test_new_abi_host_side_validation():
    """null pointers and C > 64 -> SSSEG_EINVAL (-1) before any launch: no device is touched (the pointers below are
    never dereferenced)."""
    from ssseg import native
    lib = native.lib()
    E, p, big = -1, 0x1000, 1 << 20
    prm = native.NflParams(0.25, 2, 1e-12, 1.0, 1.0, -1, 0, 1)
    pp = __import__('ctypes').addressof(prm)
    assert lib.ssseg_ce_fwd(None, None, 1, 2, 16, 1, None, None, 0, None) == E
    assert lib.ssseg_ce_fwd(p, p, 1, 65, 16, 1, p, p, big, None) == E
    assert lib.ssseg_ce_fwd(p, p, 1, 0, 16, 1, p, p, big, None) == E
    assert lib.ssseg_ce_fwd(p, p, 1, 2, 16, 2, p, p, big, None) == E          # no 'sum' for CE
    assert lib.ssseg_ce_bwd(None, None, 1, 2, 16, 1, None, None, None) == E
    assert lib.ssseg_ce_bwd(p, p, 1, 65, 16, 1, p, p, None) == E
    assert lib.ssseg_ohem_fwd(None, None, 1, 2, 16, 0.7, 10, None, None, 0, None) == E
    assert lib.ssseg_ohem_fwd(p, p, 1, 65, 16, 0.7, 10, p, p, big, None) == E
    assert lib.ssseg_ohem_bwd(None, None, 1, 2, 16, None, None, None, 0, None) == E
    assert lib.ssseg_ohem_bwd(p, p, 1, 65, 16, p, p, p, big, None) == E
    assert lib.ssseg_focal_fwd(None, None, 16, 0.25, 2.0, None, None, 0, None) == E
    assert lib.ssseg_focal_bwd(None, None, 16, 0.25, 2.0, None, None, None) == E
    assert lib.ssseg_nfl_fwd(None, None, 1, 2, 16, None, None, None, None, 0, None) == E
    assert lib.ssseg_nfl_fwd(p, p, 1, 65, 16, pp, p, p, p, big, None) == E
    assert lib.ssseg_nfl_bwd(None, None, 1, 2, 16, None, None, None, None, 0, None) == E
    assert lib.ssseg_nfl_bwd(p, p, 1, 65, 16, pp, p, p, p, big, None) == E
    assert lib.ssseg_dice_logits_fwd(None, None, 1, 2, 16, None, None, 0, None) == E
    assert lib.ssseg_dice_logits_fwd(p, p, 1, 65, 16, p, p, big, None) == E
    assert lib.ssseg_dice_logits_bwd(None, None, 1, 2, 16, None, None, None, 0, None) == E
    assert lib.ssseg_dice_logits_bwd(p, p, 1, 65, 16, p, p, p, big, None) == E
    assert lib.ssseg_dice_prob_fwd(None, None, 1, 16, 0, 1.0, None, None, 0, None) == E
    assert lib.ssseg_dice_prob_bwd(None, 1, 16, 0, 1.0, None, None, None, 0, None) == E
    assert lib.ssseg_binary_entropy_fwd(None, 16, None, None, 0, None) == E
    assert lib.ssseg_binary_entropy_bwd(None, 16, None, None, None) == E
    assert lib.ssseg_entropy_fwd(None, 1, 2, 16, None, None, 0, None) == E
    assert lib.ssseg_entropy_fwd(p, 1, 65, 16, p, p, big, None) == E
    assert lib.ssseg_entropy_bwd(None, 1, 2, 16, None, None, None) == E
    assert lib.ssseg_entropy_bwd(p, 1, 65, 16, p, p, None) == E
    assert lib.ssseg_bce_logits_red_fwd(None, None, 16, 0, None, None, 0, None) == E
    assert lib.ssseg_bce_logits_red_fwd(p, p, 16, 1, p, p, big, None) == E    # 'mean' is ssseg_bce_logits_fwd
    assert lib.ssseg_bce_logits_red_bwd(None, None, 16, 0, None, None, None) == E
    assert lib.ssseg_smooth_labels(None, None, 16, 0.9, 0.05, None) == E
    # a workspace that is too small is refused as such (SSSEG_EWORKSPACE), again on the host
    assert lib.ssseg_focal_fwd(p, p, 16, 0.25, 2.0, p, p, 8, None) == -3
    assert lib.ssseg_ohem_fwd(p, p, 1, 2, 16, 0.7, 10, p, p, 8, None) == -3
    # workspace sizes: OHEM keeps two floats per pixel on top of its partials; unknown kinds have none
    ws = lib.ssseg_segloss_workspace_bytes
    assert ws(native.LOSS_OHEM, 2, 3, 576) - ws(native.LOSS_OHEM, 2, 3, 76) == 2 * 4 * 2 * 500
    assert ws(native.LOSS_REDUCE, 16, 2, 512 * 512) == ws(native.LOSS_REDUCE, 1, 1, 1) > 0
    assert ws(99, 1, 1, 1) == 0 and ws(native.LOSS_NFL, 0, 1, 1) == 0
