"""GPU parity of the losses beyond BCE / Lovász / RMI (csrc/seglosses.hip) against the reference's golden vectors
(tests/golden/losses_ext_*.npz) and the fp64 yardstick of test_losses_ext_host.py.

Bounds: the project's loss bounds (tests/test_hip_losses.py): loss rtol 2e-5 atol 1e-7, gradient rtol 2e-4 atol 2e-8,
element by element against the golden.  The cases in FP64_BOUND do not hold them element by element (see there) and
are bound instead by: device error against the fp64 yardstick <= 4 x the reference-fp32's own error against fp64 on
that fixture + the same atol.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from test_losses_ext_host import CASES, NAN_CASES, err, nfl_kwargs, ref64

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=2e-5, atol=1e-7)
GRAD_TOL = dict(rtol=2e-4, atol=2e-8)
# cases bound against fp64 (4 x the reference's own fp32 error + atol) instead of element-wise against the golden:
#   bce_none_s1: torch's fp32 per-element BCE cancels ((1 - t) x - logsigmoid(x): for t = 0, x = -6.15 it returns
#   2.12193e-3 where fp64 gives 2.12171e-3), so 7 of the 6003 golden losses are 2e-7 off fp64 at values of 1e-3.
#   Measured: reference-fp32 vs fp64 2.386e-07, device vs fp64 2.374e-07 (loss); 2.532e-07 both (gradient).
FP64_BOUND = ('bce_none_s1',)


def _fn(name, g):
    """the public entry point of a fixture, as a callable on (x, t)"""
    import losses as L
    if name.startswith('ce_'):
        return L.DenseCrossEntropyLossWithLogits(name.split('_')[1])
    if name.startswith('ohem_'):
        return L.OhemCrossEntropy(float(g['thres']), int(g['min_kept']))
    if name.startswith('focal_'):
        return L.FocalLoss(float(g['alpha']), float(g['gamma']))
    if name.startswith('dice_'):
        return L.DiceWithLogitsLoss()
    if name.startswith('nfl_'):
        return L.NormalizedFocalLossSigmoid(**nfl_kwargs(g))
    if name == 'dicep_s1':
        return L.dice_loss
    if name.startswith('logdicep_'):
        return lambda p, t: L.log_dice_loss(p, t, gamma=float(g['gamma']))
    if name.startswith('bent_'):
        return lambda x, t: L.binary_entropy_loss(x)
    if name.startswith('ent_'):
        return lambda x, t: L.entropy_loss(x)
    if name.startswith('bce_'):
        return L.DenseBinaryCrossEntropyLossWithLogits(name.split('_')[1])
    raise KeyError(name)


def _device_run(name, dev, fn=None):
    g = golden(f'losses_ext_{name}.npz')
    x = torch.from_numpy(g['x']).to(dev).requires_grad_(True)
    t = torch.from_numpy(g['t']).to(dev) if 't' in g.files else None
    loss = (fn or _fn(name, g))(x, t)
    (loss * torch.from_numpy(g['w']).to(dev)).sum().backward()
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def _close(a, b, tol):
    return bool(np.allclose(a, b, equal_nan=True, **tol))


def _maxabs(a):
    """largest finite |a| (NaN when nothing is finite)"""
    a = np.abs(np.asarray(a, np.float64)).reshape(-1)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else float('nan')


def _grad_ok(name, grad, g):
    """the gradient comparison of a case: element-wise against the golden, or the fp64 bound"""
    if name in FP64_BOUND:
        _, g64 = ref64(name)
        try:
            return err(grad, g64) <= 4 * err(g['grad'], g64) + GRAD_TOL['atol']
        except AssertionError:   # NaN pattern differs
            return False
    return _close(grad, g['grad'], GRAD_TOL)


@pytest.mark.parametrize('name', CASES)
def test_loss_and_gradient_match_golden(hip_device, name):
    g = golden(f'losses_ext_{name}.npz')
    loss, grad = _device_run(name, hip_device)
    l64, g64 = ref64(name)
    assert loss.shape == g['loss'].shape and grad.shape == g['grad'].shape
    fin = np.isfinite(g['grad'])
    print(f'{name}: loss dev-golden {_maxabs(loss - g["loss"]):.3e}  dev-fp64 {_maxabs(loss - l64):.3e}  ref32-fp64 '
          f'{_maxabs(g["loss"] - l64):.3e} | grad dev-golden {_maxabs((grad - g["grad"])[fin]):.3e} dev-fp64 '
          f'{_maxabs((grad - g64)[fin]):.3e} ref32-fp64 {_maxabs((g["grad"] - g64)[fin]):.3e} max|grad| '
          f'{_maxabs(g["grad"][fin]):.3e} elementwise {_close(grad, g["grad"], GRAD_TOL)}')
    # NaN exactly where the golden's is
    assert np.array_equal(np.isnan(loss), np.isnan(g['loss']))
    assert np.array_equal(np.isnan(grad), np.isnan(g['grad']))
    assert (name in NAN_CASES) == bool(np.isnan(g['loss']).any())
    if name in FP64_BOUND:
        assert err(loss, l64) <= 4 * err(g['loss'], l64) + LOSS_TOL['atol']
    else:
        assert _close(loss, g['loss'], LOSS_TOL)
    assert _grad_ok(name, grad, g)
    # the comparison discriminates: a negated or a zeroed gradient fails it
    assert not _grad_ok(name, -grad, g)
    assert not _grad_ok(name, np.where(np.isnan(grad), grad, 0 * grad), g)


@pytest.mark.parametrize('min_kept,kept', [(100, 928), (1000, 1000), (5000, 1151)])
def test_ohem_kept_count_and_threshold(hip_device, min_kept, kept):
    """three regimes: threshold = thres; threshold = the order statistic; k = n - 1"""
    from ssseg import ops
    g = golden(f'losses_ext_ohem_k{min_kept}.npz')
    assert int(g['kept']) == kept
    x, t = torch.from_numpy(g['x']).to(hip_device), torch.from_numpy(g['t']).to(hip_device)
    loss, state = ops.ohem_cross_entropy(x, t, float(g['thres']), min_kept, return_state=True)
    thr, cnt = state.cpu().tolist()
    print(f'ohem k={min_kept}: threshold {thr!r} (golden {float(g["threshold"])!r}), kept {cnt}')
    assert cnt == kept
    assert abs(thr - float(g['threshold'])) <= 1e-6


def test_ohem_empty_selection_is_nan(hip_device):
    """thres = 0 with min_kept = 1 on equal logits: every pred equals the order statistic, nothing is below it"""
    import losses as L
    x = torch.zeros(1, 3, 8, 8, device=hip_device, requires_grad=True)
    t = torch.zeros(1, 3, 8, 8, device=hip_device)
    t[:, 1] = 1
    loss = L.OhemCrossEntropy(0.0, 1)(x, t)
    loss.backward()
    assert torch.isnan(loss) and float(x.grad.abs().max()) == 0.0


def test_smooth_labels(hip_device):
    import losses as L
    g = golden('losses_ext_smooth_s2.npz')
    out = L.smooth_labels(torch.from_numpy(g['t']).to(hip_device), float(g['alpha']))
    assert np.array_equal(out.cpu().numpy(), g['out'])
    assert not np.array_equal(g['t'], g['out'])


def test_nfl_k_sum_follows_the_reference(hip_device):
    import losses as L
    for name in ('nfl_default', 'nfl_s2', 'nfl_logits', 'nfl_sum'):
        g = golden(f'losses_ext_{name}.npz')
        m = L.NormalizedFocalLossSigmoid(**nfl_kwargs(g))
        ks = []
        for xk, tk in (('x', 't'), ('x2', 't2')):
            loss = m(torch.from_numpy(g[xk]).to(hip_device), torch.from_numpy(g[tk]).to(hip_device))
            ks.append(float(m._k_sum))
        print(f'{name}: k_sum {ks} golden {g["k_sum"].tolist()}')
        assert isinstance(m._k_sum, torch.Tensor) and m._k_sum.is_cuda
        np.testing.assert_allclose(ks, g['k_sum'], **LOSS_TOL)
        np.testing.assert_allclose(loss.cpu().numpy(), g['loss2'], **LOSS_TOL)

        class SW:
            def add_scalar(self, tag, value, global_step):
                self.got = (tag, value, global_step)
        sw = SW()
        m.log_states(sw, 'nfl', 3)
        assert sw.got == ('nfl_k', ks[-1], 3)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('name', CASES)
def test_bitwise_deterministic(hip_device, name):
    a, b = _device_run(name, hip_device), _device_run(name, hip_device)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize('name', ['focal_s3', 'ohem_k1000', 'dice_s1', 'nfl_default'])
def test_capture_replay_matches_eager_bitwise(hip_device, name):
    """loss = f(x, t); loss.sum().backward() captured by torch.cuda.graph after one eager warm-up, replayed twice with
    new inputs copied into the static buffers: loss and gradient are bitwise those of eager calls on those inputs (and
    for NormalizedFocal `_k_sum` advances on each replay like over the same eager calls)."""
    dev = hip_device
    g = golden(f'losses_ext_{name}.npz')
    x0, t0 = torch.from_numpy(g['x']).to(dev), torch.from_numpy(g['t']).to(dev)
    gen = torch.Generator().manual_seed(7)
    inputs = []
    for _ in range(2):
        xi = (torch.randn(x0.shape, generator=gen) * 2).to(dev)
        inputs.append((xi, t0.flip(0).contiguous() if len(inputs) else t0.flip(-1).contiguous()))
    f, f_eager = _fn(name, g), _fn(name, g)
    xs, ts = x0.clone().requires_grad_(True), t0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f(xs, ts).sum().backward()          # eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = f(xs, ts)
        loss_s.sum().backward()
    f_eager(x0.clone().requires_grad_(True), t0).sum().backward()   # the warm-up's counterpart (k_sum)
    ks = []
    for xi, ti in inputs:
        with torch.no_grad():
            xs.copy_(xi)
            ts.copy_(ti)
        graph.replay()
        xe = xi.clone().requires_grad_(True)
        le = f_eager(xe, ti)
        le.sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(loss_s.detach().cpu().numpy()), _bits(le.detach().cpu().numpy()))
        assert np.array_equal(_bits(xs.grad.cpu().numpy()), _bits(xe.grad.cpu().numpy()))
        assert float(xe.grad.abs().max()) > 0
        if name.startswith('nfl_'):
            assert float(f._k_sum) == float(f_eager._k_sum)
            ks.append(float(f._k_sum))
    if name.startswith('nfl_'):
        assert len(set(ks)) == 2 and ks[0] != float(g['k_sum'][0])


def _loss_cfg(which):
    import losses as L
    if which == 'focal_rmi':      # the reference author's last run: ..._Focal0.5-RMISigmoid0.5_...
        return [{'loss_fn': L.FocalLoss(alpha=0.5, gamma=2), 'weight': [0.5]},
                {'loss_fn': L.RMILoss(num_classes=2, rmi_radius=3, rmi_pool='avg', rmi_pool_size=4,
                                      rmi_pool_stride=4), 'weight': [0.5]}]
    return [{'loss_fn': L.OhemCrossEntropy(min_kept=1000), 'weight': [1.0]},
            {'loss_fn': L.DiceWithLogitsLoss(), 'weight': [0.125]}]


def _steps(which, graphed, device, size=64, batch=2):
    import bench
    import cowmix
    import losses as L
    import train
    from ssseg.graph import StepGraph
    model, teacher, opt, cfg = bench.build(batch, size, device)
    cfg['train']['loss'] = L.CalculateLoss(_loss_cfg(which))
    data = bench.synthetic_batches(3, batch, size, device, 0)
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    before = [p.detach().clone() for p in model.parameters()]
    model.train()
    opt.zero_grad()
    out = [train.train_step(model, teacher, opt, *data[k], 30, k, cfg) for k in range(2)]
    changed = any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    if graphed:
        g = StepGraph(lambda i, m, a, b: train.train_step(model, teacher, opt, i, m, a, b, 30, 2, cfg), *data[2])
        out.append(tuple(t.clone() for t in g(*data[2])))
    else:
        out.append(train.train_step(model, teacher, opt, *data[2], 30, 2, cfg))
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return [tuple(float(t) for t in l) for l in out], state, changed


@pytest.mark.parametrize('which', ['focal_rmi', 'ohem_dice'])
def test_train_step_with_the_new_losses(hip_device, which):
    """two eager train steps at 64^2, batch 2 with the supervised loss replaced: finite losses, parameters change; a
    third step captured through StepGraph equals the eager third step bitwise (as tests/test_graph.py does for BCE)"""
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.bfloat16)
    eager, s_e, changed = _steps(which, False, hip_device)
    graph, s_g, _ = _steps(which, True, hip_device)
    print(which, eager)
    assert changed
    assert all(np.isfinite(v) for l in eager for v in l), eager
    assert eager == graph, (eager, graph)
    for k in s_e:
        assert torch.equal(s_e[k], s_g[k]), k
