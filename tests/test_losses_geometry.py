"""GPU: the loss kernels (csrc/seglosses.hip, BCE-mean and consistency of csrc/eltwise.hip) at the grid-stride, chunk
and channel-width edges, through the public entry points, against the fp64 references of exact_losses.py.

Bounds: the project's loss bounds, imported from test_hip_losses_ext.py (loss rtol 2e-5 atol 1e-7; gradient rtol 2e-4
atol 2e-8 at every element), the gradient exactly 0.0 wherever the fp64 gradient is 0, the NaN pattern equal.  The
designs (what a probe weighs, that the fp32 CPU form itself meets these bounds, the OHEM tie groups) are proven without
a GPU in test_losses_geometry_host.py.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import exact_losses as E
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu


def entry(case):
    """the public entry point of a case as a callable on (x, t)"""
    import losses as L
    from ssseg import ops
    f, kw = case.family, case.kw
    return {
        'ce': L.DenseCrossEntropyLossWithLogits('mean'),
        'ce_none': L.DenseCrossEntropyLossWithLogits('none'),
        'ohem': L.OhemCrossEntropy(kw.get('thres', 0.7), kw.get('min_kept', 1)),
        'focal': L.FocalLoss(E.ALPHA, E.GAMMA),
        'bce_mean': ops.bce_with_logits_mean,
        'bce_sum': L.DenseBinaryCrossEntropyLossWithLogits('sum'),
        'bce_none': L.DenseBinaryCrossEntropyLossWithLogits('none'),
        'bent': lambda x, t: L.binary_entropy_loss(x),
        'ent': lambda x, t: L.entropy_loss(x),
        'nfl': L.NormalizedFocalLossSigmoid(),
        'dice': L.DiceWithLogitsLoss(),
        'dicep': L.dice_loss,
        'logdicep': lambda p, t: L.log_dice_loss(p, t, gamma=kw.get('gamma', 1.0)),
        'cons': lambda s, t: ops.consistency_loss(s, t, E.CONS_THR),
    }[f]


def device_run(case, dev, w):
    """-> (loss, gradient of (loss * w).sum(), second output or None), numpy"""
    x = torch.from_numpy(np.array(case.x)).to(dev).requires_grad_(True)
    t = None if case.t is None else torch.from_numpy(np.array(case.t)).to(dev)
    out = entry(case)(x, t)
    loss, extra = out if isinstance(out, tuple) else (out, None)
    (loss * torch.from_numpy(np.asarray(w, np.float32)).to(dev)).sum().backward()
    return (loss.detach().cpu().numpy(), x.grad.cpu().numpy(),
            None if extra is None else extra.detach().cpu().numpy())


def close(a, ref, tol):
    return bool(np.allclose(a, ref, equal_nan=True, **tol))


def _maxabs(a):
    a = np.abs(np.asarray(a, np.float64)).reshape(-1)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else float('nan')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(case, dev, twice=False):
    l64, g64, w = E.ref64(case)
    loss, grad, extra = device_run(case, dev, w)
    assert loss.shape == l64.shape and grad.shape == g64.shape
    bad = ~np.isclose(grad, g64, equal_nan=True, **GRAD_TOL)
    print(f'{case.name} {case.x.shape}: loss dev-fp64 {_maxabs(loss - l64):.3e} of {_maxabs(l64):.6e} | grad dev-fp64 '
          f'{_maxabs(grad - g64):.3e} of {_maxabs(g64):.3e}, {int(bad.sum())} of {bad.size} entries out of bound'
          + (f', first at {tuple(int(i) for i in np.argwhere(bad)[0])}: {grad[bad][0]!r} vs {g64[bad][0]!r}'
             if bad.any() else ''))
    assert np.array_equal(np.isnan(loss), np.isnan(l64))
    assert np.array_equal(np.isnan(grad), np.isnan(g64))
    assert close(loss, l64, LOSS_TOL)
    assert not bad.any()
    assert np.all(grad[g64 == 0] == 0)
    if twice:   # a race in the read-back of the partials would show here
        loss2, grad2, _ = device_run(case, dev, w)
        assert np.array_equal(bits(loss), bits(loss2)) and np.array_equal(bits(grad), bits(grad2))
    return loss, grad, extra


# ---- probe cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.PROBE_CASES)
def test_probe_case(hip_device, name):
    from ssseg import ops
    case = E.probe_case(name)
    _, g64, _ = E.ref64(case)
    loss, grad, extra = check(case, hip_device, twice=True)
    if _maxabs(g64) > 2.0 ** -9:   # the comparison discriminates: a negated or a zeroed gradient fails it
        assert not close(-grad, g64, GRAD_TOL) and not close(0 * grad, g64, GRAD_TOL)
    if case.family == 'ohem':
        x, t = (torch.from_numpy(np.array(a)).to(hip_device) for a in (case.x, case.t))
        _, state = ops.ohem_cross_entropy(x, t, case.kw['thres'], case.kw['min_kept'], return_state=True)
        thr, kept = state.cpu().tolist()
        print(f'{name}: threshold {thr!r}, kept {kept}')
        assert kept == len(case.sites) and thr == float(np.float32(case.kw['thres']))
    if case.family == 'cons':
        print(f'{name}: confident fraction {extra!r}, count {case.kw["count"]} of {case.npix}')
        assert extra.dtype == np.float32 and extra == np.float32(case.kw['count'] / case.npix)


# ---- the channel-width sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', E.WIDTHS)
@pytest.mark.parametrize('family', E.SWEEP_FAMILIES)
def test_channel_width(hip_device, family, C):
    for hw in E.SWEEP_HW:
        check(E.sweep_case(family, C, hw), hip_device)


def test_65_channels_are_refused(hip_device):
    import losses as L
    x = torch.zeros(2, 65, 7, 9, device=hip_device)
    for f in (L.DenseCrossEntropyLossWithLogits(), L.OhemCrossEntropy(), L.DiceWithLogitsLoss()):
        with pytest.raises(ValueError, match='65 channels'):
            f(x, x)
    with pytest.raises(ValueError, match='65 channels'):
        L.entropy_loss(x)


# ---- the second round of the element-wise and backward kernels ---------------------------------------------------
@pytest.mark.parametrize('family', E.GRID_FAMILIES)
def test_second_grid_round(hip_device, family):
    """1,048,869 pixels: every element of the gradient (and of the 'none' outputs) against fp64"""
    check(E.grid_case(family), hip_device)


def test_smooth_labels_second_round(hip_device):
    import losses as L
    t = torch.from_numpy(np.array(E.grid_case('ce').t))
    out = L.smooth_labels(t.to(hip_device), 0.1).cpu()
    assert torch.equal(out, t * (1 - 0.1) + 0.1 / t.size(1))
    assert not torch.equal(out, t)


# ---- the OHEM radix select ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1, 2])
def test_ohem_selection(hip_device, which):
    """every rank of the design (inside a tie group, on its first and last element, clamped to npix - 1) under one of
    the three thresholds: the kept count is the integer the group sizes give, the threshold the group's value"""
    from ssseg import ops
    d = E.ohem_design()
    thres = d.thresholds[which]
    x, t = (torch.from_numpy(np.array(a)).to(hip_device) for a in (d.x, d.t))
    got = []
    for k in d.ranks():
        loss, state = ops.ohem_cross_entropy(x, t, thres, k, return_state=True)
        got.append((k, float(loss)) + tuple(state.cpu().tolist()))
    fails = []
    for k, loss, thr, kept in got:
        e_thr, e_kept, e_loss = d.expected(k, thres)
        ok = (kept == e_kept and abs(thr - e_thr) <= 1e-6
              and close(np.float64(loss), np.float64(e_loss), LOSS_TOL))
        print(f'thres {thres} k {k}: kept {kept} (expected {e_kept}) threshold {thr!r} ({e_thr!r}) loss {loss!r} '
              f'({e_loss!r}){"" if ok else "  <-- FAIL"}')
        if not ok:
            fails.append(k)
    assert not fails
    # the gradient of one rank inside the largest tie group, every element
    k = d.cum[5] - 1234
    check(E.Case(f'ohem_select_{which}', 'ohem', d.x, d.t, kw={'thres': thres, 'min_kept': k}), hip_device, twice=True)
