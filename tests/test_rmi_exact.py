"""The RMI loss kernels (csrc/rmi.hip), stage by stage, against the host restatements of tests/exact_rmi.py.

ssseg_rmi_fwd / ssseg_rmi_bwd are called through ssseg.native on the test's own workspace, prefilled with 0xFF bytes
(a NaN in every fp32 and fp64 slot, so an element a kernel leaves unwritten cannot pass).  The workspace is decoded by
the restated layout -- whose total must equal ssseg_rmi_workspace_bytes -- and every stage is compared with ITS OWN
inputs as the device produced them (exact_rmi.check_all): bit equality where the arithmetic is fixed, a derived
per-element bound elsewhere, and for the D x D solve 16 x the measured error of two fp64 host routes against long double.
Each geometry of exact_rmi.GEOS (the smallest at which one edge of the launch geometry is live; test_rmi_exact_host.py
asserts the edge) runs once on designed and once on random operands.  Every test prints its figures before it asserts."""
import math

import numpy as np
import pytest
import torch

import exact_rmi as R
from exact_step import same_bits

pytestmark = pytest.mark.gpu

IDS = [R.geo_id(c) for c in R.GEOS]


def _run(dev, case, kind, want_grad=1, backward=True):
    """forward (+ backward) on (case, kind): the decoded workspace, loss, gx and the raw workspace bytes"""
    from ssseg import native as N
    g = R.Geo(case)
    x, t, gout = R.operands(case, kind)
    nb = int(N.lib().ssseg_rmi_workspace_bytes(*g.args))
    xd, td = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(t)).to(dev)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    loss = torch.full((1,), float('nan'), device=dev)
    gx = torch.full_like(xd, float('nan'))
    N.call('ssseg_rmi_fwd', xd.data_ptr(), td.data_ptr(), *g.args, want_grad, loss.data_ptr(), ws.data_ptr(), nb,
           N.stream())
    if want_grad and backward:
        go = torch.tensor([gout], dtype=torch.float32, device=dev)
        N.call('ssseg_rmi_bwd', xd.data_ptr(), *g.args, go.data_ptr(), gx.data_ptr(), ws.data_ptr(), nb, N.stream())
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    run = R.decode(raw, g, nb)
    run.update(loss=loss.cpu().numpy()[0], gx=gx.cpu().numpy(), raw=raw)
    return run


def _same_run(a, b, what):
    same_bits(np.asarray(a['loss']).reshape(1), np.asarray(b['loss']).reshape(1), f'{what}: loss')
    same_bits(a['gx'].view(np.uint32), b['gx'].view(np.uint32), f'{what}: gx')
    same_bits(a['raw'], b['raw'], f'{what}: workspace')


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', R.GEOS, ids=IDS)
def test_rmi_stages(hip_device, case, kind):
    """Stages 1-8 of exact_rmi on the device's workspace, the run-to-run bit equality of loss, gx and the whole
    workspace, and the forward without the backward coefficients (want_grad = 0): the same loss and rmi bits.  At
    P = 1 also the closed form.  On the 726 x 726 geometry the long double covariance check runs on series 0 (both
    series go through every other stage)."""
    what = f'{R.geo_id(case)} {kind}'
    g = R.Geo(case)
    run = _run(hip_device, case, kind)
    _same_run(run, _run(hip_device, case, kind), f'{what}: second run')
    fwd = _run(hip_device, case, kind, want_grad=0)
    same_bits(np.asarray(fwd['loss']).reshape(1), np.asarray(run['loss']).reshape(1), f'{what}: want_grad 0 loss')
    same_bits(fwd['rmi'], run['rmi'], f'{what}: want_grad 0 rmi')
    R.check_all(run, case, kind, what, cov_series=[0] if case == R.BIG else None)
    if case == R.P_ONE:
        cf = R.closed_form_p1(g)
        err = float(np.abs(run['rmi'] - cf).max())
        bound = R.closed_form_bound(g)
        print(f'{what}: closed form {cf!r}: worst error {err:.3e} bound {bound:.3e}; loss {float(run["loss"])!r}')
        assert err <= bound
        assert (run['coef'] == 0).all() and (run['gp'] == 0).all() and (run['gx'] == 0).all()
        want = np.float32(0)
        for _ in range(g.ncls):
            want = np.float32(want + np.float32(np.float32(cf) / np.float32(g.D)))
        assert abs(float(run['loss']) - float(want)) <= 2.0 ** -22 * abs(float(want))


def test_rmi_absent_class(hip_device):
    """Label channel 1 all zero: for its series Lc = M = 0 exactly, so K = Q = 0, the gradient of that channel is
    exactly 0, and rmi = logdet(aI) / 1 is free of the probabilities: the same bits after that channel's logits are
    redrawn.  Every stage check runs as usual."""
    case = R.SPECIAL_GEO
    g = R.Geo(case)
    run = _run(hip_device, case, 'absent')
    other = _run(hip_device, case, 'absent2')
    R.check_all(run, case, 'absent', 'absent class')
    sel = np.arange(g.NC) % g.C == 1
    Lc, S, M = R.sum_chunks(run['part'], g)
    print('absent class: rmi', run['rmi'], 'after redrawing the logits', other['rmi'], 'closed form',
          R.closed_form_p1(g))
    assert (Lc[sel] == 0).all() and (M[sel] == 0).all() and (S[sel] != 0).any()
    assert (run['coef'][sel] == 0).all() and (run['gp'][sel] == 0).all()
    assert (run['gx'].reshape(g.NC, -1)[sel] == 0).all() and (run['gx'].reshape(g.NC, -1)[~sel] != 0).any()
    same_bits(run['rmi'][sel], other['rmi'][sel], 'absent class: rmi after redrawing the logits')
    assert not np.array_equal(run['pp'][sel], other['pp'][sel])
    cf = R.closed_form_p1(g)
    assert np.abs(run['rmi'][sel] - cf).max() <= R.closed_form_bound(g)
    assert math.isfinite(float(run['loss'])) and np.isfinite(run['gx']).all()


def test_rmi_saturated_channel(hip_device):
    """Logit channel 0 all +30: every probability of the channel is exactly 1, the centred values are 0, S = aI and
    M = 0.  Loss and gradient are finite, the channel's gradient exactly 0."""
    case = R.SPECIAL_GEO
    g = R.Geo(case)
    run = _run(hip_device, case, 'saturated')
    R.check_all(run, case, 'saturated', 'saturated channel')
    sel = np.arange(g.NC) % g.C == 0
    Lc, S, M = R.sum_chunks(run['part'], g)
    print('saturated channel: rmi', run['rmi'], 'loss', float(run['loss']))
    assert (run['pp'][sel] == 1).all() and (S[sel] == 0).all() and (M[sel] == 0).all() and (Lc[sel] != 0).any()
    assert (run['coef'][sel] == 0).all() and (run['gx'].reshape(g.NC, -1)[sel] == 0).all()
    assert math.isfinite(float(run['loss'])) and np.isfinite(run['gx']).all() and np.isfinite(run['rmi']).all()
