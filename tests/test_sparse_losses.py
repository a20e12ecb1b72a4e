"""GPU: the label-map losses (ssseg_ce_labels_*, ssseg_ohem_labels_* in csrc/seglosses.hip) through their public
entry points, and the training step, validation and captured step on label-map batches.

1. Bit for bit against the dense kernels on one-hot targets (no void, no weight, no smoothing), every channel bucket.
2. Against the fp64 restatement (tests/sparse_ref.py, pinned on the host to F.cross_entropy and to the reference's
   fixtures).  Bounds: the project's (test_hip_losses_ext.py): loss rtol 2e-5 atol 1e-7, gradient rtol 2e-4 atol 2e-8
   at every element; where torch's own fp32 CPU run of the same case misses them, 4 x its error against fp64 + the atol
   (that file's rule).
3. The launch edges on designed operands (exact_losses.py's probe principle: a void pixel contributes exactly 0, so
   everything but a few probes is void and a lost or doubled probe moves the scalar by far more than the bound).
4. Determinism and graph capture.  5. The trainer end to end.
Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as R
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64
RED_SPAN = 256 * 1024     # RED_THREADS * RED_BLOCKS: one round of a reduction (and of the OHEM per-pixel kernel)
GRID_SPAN = 256 * 4096    # 256 threads * the default grid cap: one round of a backward
BUCKETS = [2, 3, 7, 13, 19, 40, 64]   # one C per Soft<CM> instantiation (CM = 2, 4, 8, 16, 32, 64, 64)


def _maxabs(a):
    a = np.abs(np.asarray(a, np.float64)).reshape(-1)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def _close(a, ref, tol):
    return bool(np.allclose(a, ref, equal_nan=True, **tol))


def _bounded(dev, r64, r32, tol):
    """element-wise at the project's bound, or, where torch's fp32 itself misses it, 4 x its error + atol"""
    dev, r64 = np.asarray(dev, np.float64), np.asarray(r64, np.float64)
    if not np.array_equal(np.isnan(dev), np.isnan(r64)):
        return False
    if r32 is None or _close(r32, r64, tol):
        return _close(dev, r64, tol)
    return _maxabs(dev - r64) <= 4 * _maxabs(np.asarray(r32, np.float64) - r64) + tol['atol']


def _logits(shape, seed, scale=2.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _labels(shape, C, seed, void=0.0, ignore=255):
    g = torch.Generator().manual_seed(seed + 77)
    y = torch.randint(0, C, shape, generator=g)
    if 0 <= ignore < C:
        y[y == ignore] = (ignore + 1) % C
    if void:
        y[torch.rand(shape, generator=g) < void] = ignore
    return y


def _dev_ce(x, y, dev, up, w=None, **kw):
    """-> (loss, gradient of (loss * up).sum()) as numpy"""
    from ssseg import ops
    xd = x.detach().to(dev).requires_grad_(True)
    loss = ops.cross_entropy_labels(xd, y.to(dev), None if w is None else w.to(dev), **kw)
    (loss * (up.to(dev) if torch.is_tensor(up) else up)).sum().backward()
    return loss.detach().cpu().numpy(), xd.grad.cpu().numpy()


def _ref_ce(x, y, up, dtype, w=None, torch_fn=False, **kw):
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    wr = None if w is None else w.to(dtype)
    if torch_fn:    # torch itself (it raises on labels outside [0, C): those are void by definition here)
        C, ign = x.shape[1], kw['ignore_index']
        yl = y.long()
        yl = torch.where((yl < 0) | (yl >= C), torch.full_like(yl, ign), yl)
        loss = F.cross_entropy(xr, yl, wr, ignore_index=ign, reduction=kw['reduction'],
                               label_smoothing=kw['label_smoothing'])
    else:
        loss = R.ce_labels64(xr, y, wr, **kw)
    g, = torch.autograd.grad((loss * (up.to(dtype) if torch.is_tensor(up) else up)).sum(), xr)
    return loss.detach().numpy(), g.numpy()


# ---- 1. bit for bit against the dense kernels --------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int64], ids=['u8', 'i64'])
@pytest.mark.parametrize('C', BUCKETS)
def test_bitwise_against_the_dense_kernels(hip_device, C, dtype):
    from ssseg import ops
    B, H, W = 2, 17, 31
    x = _logits((B, C, H, W), C).to(hip_device)
    y = _labels((B, H, W), C, C)
    t = F.one_hot(y, C).permute(0, 3, 1, 2).float().contiguous().to(hip_device)
    y = y.to(dtype).to(hip_device)
    up = torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)).to(hip_device)

    def grad(fn, mul):
        xr = x.clone().requires_grad_(True)
        out = fn(xr)
        (out * mul).sum().backward()
        return out.detach(), xr.grad

    ls, gs = grad(lambda v: ops.cross_entropy_labels(v, y, reduction='none'), up)
    ld, gd = grad(lambda v: ops.dense_cross_entropy(v, t, 'none'), up)
    ms, gms = grad(lambda v: ops.cross_entropy_labels(v, y, reduction='mean'), 0.7312)
    md, gmd = grad(lambda v: ops.dense_cross_entropy(v, t, 'mean'), 0.7312)
    print(f'C={C} {dtype}: none values equal {torch.equal(ls, ld)} grads equal {torch.equal(gs, gd)}; mean '
          f'{float(ms)!r} / {float(md)!r} grads equal {torch.equal(gms, gmd)}')
    assert torch.isfinite(ld).all() and gd.any() and gmd.any()
    assert torch.equal(ls, ld) and torch.equal(gs, gd) and torch.equal(gms, gmd)
    assert _close(ms.cpu().numpy(), md.cpu().numpy(), LOSS_TOL)
    for thresh, min_kept in ((0.7, 100), (0.0, B * H * W // 3)):
        state = {}

        def sparse(v):
            out, state['s'] = ops.ohem_cross_entropy_labels(v, y, thresh, min_kept, return_state=True)
            return out

        def dense(v):
            out, state['d'] = ops.ohem_cross_entropy(v, t, thresh, min_kept, return_state=True)
            return out
        os_, gos = grad(sparse, 0.7312)
        od, god = grad(dense, 0.7312)
        print(f'  ohem thresh {thresh} min_kept {min_kept}: state {state["s"].tolist()} / {state["d"].tolist()} loss '
              f'{float(os_)!r} / {float(od)!r}')
        assert torch.equal(state['s'], state['d']) and 0 < float(state['d'][1]) < B * H * W
        assert torch.equal(os_, od) and torch.equal(gos, god) and god.any()


# ---- 2. against the fp64 restatement -----------------------------------------------------------------------------
W5 = torch.tensor([0.5, 2.0, 1.0, 0.25, 3.0])
CE_CASES = [(w, eps, red, ign, dt, var)
            for i, (w, eps, red) in enumerate((w, eps, red) for w in (False, True) for eps in (0.0, 0.1)
                                              for red in ('mean', 'sum', 'none'))
            for ign, dt, var in [((255, -100, 0)[i % 3], (torch.uint8, torch.int64)[(i % 3) != 0], 'void')]]
CE_CASES += [(True, 0.1, 'mean', 255, torch.uint8, 'image_void'), (False, 0.0, 'mean', 0, torch.int64, 'image_void'),
             (True, 0.1, 'sum', 255, torch.uint8, 'out_of_range'),
             (False, 0.0, 'none', -100, torch.int64, 'out_of_range'),
             (True, 0.0, 'mean', 255, torch.uint8, 'out_of_range')]


@pytest.mark.parametrize('weighted,eps,reduction,ignore,dtype,variant', CE_CASES)
def test_ce_against_fp64(hip_device, weighted, eps, reduction, ignore, dtype, variant):
    B, C, H, W = 3, 5, 17, 31
    x = _logits((B, C, H, W), 11)
    y = _labels((B, H, W), C, 12, void=0.15, ignore=ignore)
    if variant == 'image_void':
        y[1] = ignore
    if variant == 'out_of_range':      # labels that are neither a class nor the ignore value: void
        g = torch.Generator().manual_seed(3)
        y[torch.rand(B, H, W, generator=g) < 0.1] = 200 if dtype == torch.uint8 else 10 ** 12
        y[torch.rand(B, H, W, generator=g) < 0.05] = 5 if dtype == torch.uint8 else -7
    y = y.to(dtype)
    w = W5 if weighted else None
    up = torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) if reduction == 'none' else 0.7312
    kw = dict(ignore_index=ignore, reduction=reduction, label_smoothing=eps)
    l64, g64 = _ref_ce(x, y, up, F64, w, **kw)
    l32, g32 = _ref_ce(x, y, up, torch.float32, w, torch_fn=True, **kw)
    loss, grad = _dev_ce(x, y, hip_device, up, w, **kw)
    nvoid = int(((y.long() == ignore) | (y.long() < 0) | (y.long() >= C)).sum())
    print(f'{variant} w={weighted} eps={eps} {reduction} ignore={ignore} {dtype}: {nvoid} void of {y.numel()}; loss '
          f'dev-fp64 {_maxabs(loss - l64):.3e} torch32-fp64 {_maxabs(l32 - l64):.3e} of {_maxabs(l64):.3e} | grad '
          f'dev-fp64 {_maxabs(grad - g64):.3e} torch32-fp64 {_maxabs(g32 - g64):.3e} of {_maxabs(g64):.3e}; torch32 '
          f'element-wise loss {_close(l32, l64, LOSS_TOL)} grad {_close(g32, g64, GRAD_TOL)}')
    assert 0 < nvoid < y.numel() and loss.shape == l64.shape and loss.dtype == np.float32
    assert _bounded(loss, l64, l32, LOSS_TOL)
    assert _bounded(grad, g64, g32, GRAD_TOL)
    assert np.all(grad[g64 == 0] == 0) and (g64 == 0).any()        # void pixels: exact zeros
    assert not _bounded(-grad, g64, g32, GRAD_TOL) and not _bounded(0 * grad, g64, g32, GRAD_TOL)


@pytest.mark.parametrize('name', ['s1', 'c19', 'novoid', 'allvoid'])
def test_default_path_against_the_reference_fixtures(hip_device, name):
    """losses.CrossEntropyLossWithLogits() is the reference's lovasz.xloss"""
    import losses as L
    from conftest import golden
    g = golden(f'sparse_ce_{name}.npz')
    x = torch.from_numpy(g['x']).to(hip_device).requires_grad_(True)
    loss = L.CrossEntropyLossWithLogits()(x, torch.from_numpy(g['y']).to(hip_device))
    (loss * float(g['w'])).backward()
    loss, grad = loss.detach().cpu().numpy(), x.grad.cpu().numpy()
    print(f'{name}: loss {loss!r} golden {g["loss"]!r} grad dev-golden {_maxabs(grad - g["grad"]):.3e}')
    assert _close(loss, g['loss'], LOSS_TOL) and _close(grad, g['grad'], GRAD_TOL)
    assert np.all(grad[g['grad'] == 0] == 0)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
@pytest.mark.parametrize('empty', ['nan', 'zero'])
def test_everything_void(hip_device, empty, reduction, weighted):
    x = _logits((2, 4, 9, 11), 1)
    y = torch.full((2, 9, 11), 255, dtype=torch.uint8)
    loss, grad = _dev_ce(x, y, hip_device, 0.7312, W5[:4] if weighted else None, reduction=reduction,
                         label_smoothing=0.1 if weighted else 0.0, empty=empty)
    print(f'all void, {reduction}, empty={empty}, weighted={weighted}: loss {loss!r} max|grad| {np.abs(grad).max()!r}')
    if reduction == 'mean' and empty == 'nan':
        assert np.isnan(loss)
    else:
        assert np.array_equal(loss, np.zeros_like(loss))
    assert not np.isnan(grad).any() and not grad.any()


# ---- OHEM against the restatement ------------------------------------------------------------------------------
def _dev_ohem(x, y, dev, thresh, min_kept, ignore=255):
    from ssseg import ops
    xd = x.detach().to(dev).requires_grad_(True)
    loss, state = ops.ohem_cross_entropy_labels(xd, y.to(dev), thresh, min_kept, ignore, return_state=True)
    (loss * 0.7312).backward()
    thr, kept = state.cpu().tolist()
    return loss.detach().cpu().numpy(), xd.grad.cpu().numpy(), thr, kept


def _check_ohem(name, x, y, dev, thresh, min_kept, ignore=255, want_kept=None):
    thr64, sel, n = R.ohem_labels_state64(x.double(), y, thresh, min_kept, ignore)
    xr = x.double().requires_grad_(True)
    l64 = R.ohem_labels64(xr, y, thresh, min_kept, ignore)
    g64, = torch.autograd.grad(l64 * 0.7312, xr)
    l64, g64 = l64.detach().numpy(), g64.numpy()
    loss, grad, thr, kept = _dev_ohem(x, y, dev, thresh, min_kept, ignore)
    print(f'{name}: thresh {thresh} min_kept {min_kept} n_valid {n}: threshold {thr!r} ({thr64!r}) kept {kept} '
          f'({int(sel.sum())}) loss {loss!r} ({l64!r}) grad dev-fp64 {_maxabs(grad - g64):.3e} of {_maxabs(g64):.3e}')
    assert kept == int(sel.sum())
    if want_kept is not None:
        assert kept == want_kept
    assert thr == thr64 == float('inf') if n == 0 else abs(thr - thr64) <= 1e-6
    assert _close(loss, l64, LOSS_TOL) and _close(grad, g64, GRAD_TOL)
    assert np.all(grad[g64 == 0] == 0) and not np.isnan(grad).any()
    return kept


def _levels(a, C=2):
    """logits [1, C, n] whose softmax at class 0 is sigmoid(a) for C == 2 (the other channels 0)"""
    x = torch.zeros(1, C, a.numel())
    x[0, 0] = a
    return x


def test_ohem_against_fp64_with_void(hip_device):
    B, C, H, W = 3, 5, 17, 31
    x = _logits((B, C, H, W), 21)
    y = _labels((B, H, W), C, 22, void=0.3).to(torch.uint8)
    y[1] = 255                                                   # one image entirely void
    n = int((y != 255).sum())
    for thresh, min_kept in ((0.7, 50), (0.0, n // 2), (0.9, n - 1), (0.0, n), (0.0, 10 ** 9)):
        _check_ohem('random', x, y, hip_device, thresh, min_kept)
    x0 = _logits((2, 3, 8, 8), 2)
    kept = _check_ohem('all void', x0, torch.full((2, 8, 8), 255, dtype=torch.uint8), hip_device, 0.7, 10)
    assert kept == 0
    loss = _dev_ohem(x0, torch.full((2, 8, 8), 255, dtype=torch.uint8), hip_device, 0.7, 10)[0]
    assert np.isnan(loss)
    y2 = _labels((2, 8, 8), 3, 4, void=0.3, ignore=1)           # the ignore value inside the range, int64 labels
    _check_ohem('ignore inside', x0, y2, hip_device, 0.0, 20, ignore=1)


def test_ohem_order_statistic_edges(hip_device):
    """designed operands: pred = sigmoid(level), levels 0.05 apart (preds differ by > 2e-3: fp32 and fp64 order them
    alike), label 0 or void"""
    n = 300
    g = torch.Generator().manual_seed(8)
    # (a) distinct ascending levels over the valid pixels in memory order, void pixels in between and at the end: the
    # statistic of rank n_valid - 1 is the last valid pixel
    y = torch.zeros(1, n, dtype=torch.int64)
    y[0, torch.rand(n, generator=g) < 0.3] = 255
    y[0, -20:] = 255
    valid = y[0] != 255
    nv = int(valid.sum())
    a = torch.zeros(n)
    a[valid] = -3.0 + 0.05 * torch.arange(nv, dtype=torch.float32)
    a[~valid] = 9.0                                              # what a void pixel holds must not matter
    x = _levels(a)
    last = int(valid.nonzero()[-1])
    _check_ohem('last valid pixel', x, y, hip_device, 0.0, nv - 1, want_kept=nv - 1)
    xd = x.detach().to(hip_device).requires_grad_(True)
    from ssseg import ops
    ops.ohem_cross_entropy_labels(xd, y.to(hip_device), 0.0, nv - 1).backward()
    assert not xd.grad[0, :, last].any() and xd.grad[0, :, int(valid.nonzero()[-2])].any()
    # (b) min_kept > n_valid clamps to n_valid - 1 (an unclamped rank would land on a void key: everything kept)
    for mk in (nv, nv + 1, n - 1, n, 10 ** 7):
        _check_ohem('clamped', x, y, hip_device, 0.0, mk, want_kept=nv - 1)
    _check_ohem('rank 0', x, y, hip_device, 0.0, 0, want_kept=0)
    # (c) tie groups: every level four times, the largest one six times, right below the void keys
    lev = -2.0 + 0.05 * (torch.arange(nv) // 4).float()
    top = float(lev.max())
    lev[-6:] = top
    a2 = torch.zeros(n)
    a2[valid] = lev[torch.randperm(nv, generator=g)]
    x2 = _levels(a2)
    ntop, srt = int((lev == top).sum()), lev.sort()[0]
    assert ntop == 6

    def want(k):     # the pixels strictly below the level of rank k
        return int((lev < srt[min(k, nv - 1)]).sum())
    assert want(nv - 1) == want(nv - ntop) == nv - ntop and want(nv - ntop - 1) < nv - ntop - 1 and want(9) == 8
    _check_ohem('top tie', x2, y, hip_device, 0.0, nv - 1, want_kept=nv - ntop)
    _check_ohem('top tie, clamped', x2, y, hip_device, 0.0, 10 ** 6, want_kept=nv - ntop)
    _check_ohem('top tie, first of the group', x2, y, hip_device, 0.0, nv - ntop, want_kept=nv - ntop)
    _check_ohem('below the top tie', x2, y, hip_device, 0.0, nv - ntop - 1, want_kept=want(nv - ntop - 1))
    _check_ohem('inner tie', x2, y, hip_device, 0.0, 9, want_kept=8)
    _check_ohem('thresh above every pred', x2, y, hip_device, 1.0, 5, want_kept=nv)


# ---- 3. launch edges on designed operands ------------------------------------------------------------------------
def _probe_case(B, C, HW, sites, seed, dtype=torch.uint8):
    """everything void but the probes at the flat pixel indices `sites` (distinct classes and logits per probe); the
    void pixels carry large logits that must not be read into anything"""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, C, HW), 30.0)
    y = torch.full((B * HW,), 255, dtype=torch.int64)
    for j, q in enumerate(sites):
        b, p = divmod(q, HW)
        x[b, :, p] = 2 * torch.randn(C, generator=g) + 0.37 * j
        y[q] = j % C
    return x, y.view(B, HW).to(dtype)


def _check_probes(name, x, y, sites, dev, w=None, eps=0.0, ohem=True):
    B, C, HW = x.shape
    for red in ('mean', 'sum'):
        kw = dict(ignore_index=255, reduction=red, label_smoothing=eps)
        l64, g64 = _ref_ce(x, y, 0.7312, F64, w, **kw)
        xd = x.detach().to(dev).requires_grad_(True)
        from ssseg import ops
        loss = ops.cross_entropy_labels(xd, y.to(dev), None if w is None else w.to(dev), **kw)
        (loss * 0.7312).backward()
        nz = int((xd.grad != 0).any(1).sum())
        b, p = np.divmod(np.asarray(sites), HW)
        gp, gp64 = xd.grad[b, :, p].cpu().numpy(), g64[b, :, p]
        print(f'{name} {tuple(x.shape)} {red}: loss {float(loss.detach())!r} fp64 {float(l64)!r}; pixels with a '
              f'gradient {nz} '
              f'of {len(sites)} probes; probe grad dev-fp64 {_maxabs(gp - gp64):.3e} of {_maxabs(gp64):.3e}')
        assert _close(loss.detach().cpu().numpy(), l64, LOSS_TOL)
        assert nz == len(sites) and _close(gp, gp64, GRAD_TOL)
    none = ops.cross_entropy_labels(x.to(dev), y.to(dev), None if w is None else w.to(dev), 255, 'none', eps)
    n64 = R.ce_labels64(x.double(), y, None if w is None else w.double(), 255, 'none', eps)
    assert int((none != 0).sum()) == len(sites) and _close(none.cpu().numpy(), n64.numpy(), LOSS_TOL)
    if ohem:
        k = len(sites) // 2
        _check_ohem(name, x, y, dev, 0.0, k, want_kept=k)
        _check_ohem(name + ' clamped', x, y, dev, 0.0, 10 ** 9, want_kept=len(sites) - 1)


def test_sample_boundary_inside_a_wavefront(hip_device):
    HW, B = 527, 3
    sites = [0, 63, 64, 255, 256, 526, 527, 528, 575, 576, 1053, 1054, 1055, 1580]
    x, y = _probe_case(B, 5, HW, sites, 31)
    _check_probes('HW 527', x, y, sites, hip_device, w=W5, eps=0.1)
    _check_probes('HW 527 plain', x, y, sites, hip_device)


def test_second_round_of_every_reduction(hip_device):
    """npix just above 256 * 1024: the valid pixels sit in the second round of the grid-stride loops only"""
    n = RED_SPAN + 300
    sites = [RED_SPAN, RED_SPAN + 1, RED_SPAN + 63, RED_SPAN + 64, RED_SPAN + 255, RED_SPAN + 256, n - 1]
    x, y = _probe_case(1, 3, n, sites, 32)
    _check_probes('second round', x, y, sites, hip_device, w=W5[:3], eps=0.1)
    x, y = _probe_case(2, 3, n // 2, sites, 33, dtype=torch.int64)      # the same sites, now in the second sample
    _check_probes('second round, two samples', x, y, sites, hip_device)


def test_second_round_of_the_backward(hip_device):
    n = GRID_SPAN + 70
    sites = [0, GRID_SPAN - 1, GRID_SPAN, GRID_SPAN + 1, GRID_SPAN + 64, n - 1]
    x, y = _probe_case(1, 2, n, sites, 34)
    _check_probes('backward second round', x, y, sites, hip_device)


def test_more_than_256_partials(hip_device):
    """300 blocks leave 300 partials: the final block's threads take a second one; probes in blocks 3, 255 - 299"""
    n = 256 * 300 - 9
    sites = [256 * 3 + 5, 256 * 255 + 255, 256 * 256, 256 * 256 + 1, 256 * 280 + 17, n - 1]
    x, y = _probe_case(1, 4, n, sites, 35)
    _check_probes('300 partials', x, y, sites, hip_device, w=W5[:4], eps=0.1)


# ---- 4. determinism and graph capture ----------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal_and_a_captured_graph_replays(hip_device):
    from ssseg import ops
    from ssseg.graph import StepGraph
    B, C, H, W = 2, 19, 33, 47
    w = torch.rand(C, generator=torch.Generator().manual_seed(1)).to(hip_device) + 0.5

    def data(seed):
        return (_logits((B, C, H, W), seed).to(hip_device),
                _labels((B, H, W), C, seed, void=0.2).to(torch.uint8).to(hip_device))

    def fn(x, y):
        xr = x.detach().requires_grad_(True)
        ce = ops.cross_entropy_labels(xr, y, w, 255, 'mean', 0.1)
        oh, state = ops.ohem_cross_entropy_labels(xr, y, 0.7, 200, return_state=True)
        g, = torch.autograd.grad(ce + 2 * oh, xr)
        return ce, oh, state.clone(), g

    a, b = data(1), data(2)
    first = [t.clone() for t in fn(*a)]
    again = [t.clone() for t in fn(*a)]
    eager_b = [t.clone() for t in fn(*b)]
    graph = StepGraph(fn, *a, warmup=1)
    replay_b = [t.clone() for t in graph(*b)]
    replay_a = [t.clone() for t in graph(*a)]
    torch.cuda.synchronize()
    for name, out in (('eager a', first), ('eager b', eager_b), ('replay b', replay_b)):
        print(name, [float(t.detach()) for t in out[:2]], out[2].tolist())
    assert all(torch.isfinite(t).all() for t in first + eager_b) and first[3].any()
    assert not torch.equal(first[0], eager_b[0])
    for u, v in zip(first, again):
        assert torch.equal(u, v)
    for u, v in zip(eager_b, replay_b):
        assert torch.equal(u, v)
    for u, v in zip(first, replay_a):
        assert torch.equal(u, v)


# ---- 5. end to end -------------------------------------------------------------------------------------------------
from test_multiclass import _Spy, _small_pair, _tcfg, fp32_compute  # noqa: E402,F401  (the small 5-class models)

NC = 5


def _loss(label_map):
    import losses as L
    ce = L.CrossEntropyLossWithLogits() if label_map else L.DenseCrossEntropyLossWithLogits('mean')
    return L.CalculateLoss([{'loss_fn': ce, 'weight': [0.5]},
                            {'loss_fn': L.LovaszSoftmaxLossWithLogits(ignore=255), 'weight': [0.5]}])


def _dataset(label_map, void=0.0, length=12, seed=5):
    from data.synthetic import SyntheticSegDataset
    return SyntheticSegDataset(length=length, size=64, seed=seed, blob_sigma=4.0, num_classes=NC, label_map=label_map,
                               void_fraction=void)


def _batches(ds, steps, dev):
    g = torch.Generator().manual_seed(17)
    unl = torch.rand(2 * steps, 2, 3, 64, 64, generator=g)
    out = []
    for k in range(steps):
        s = [ds[2 * k], ds[2 * k + 1]]
        out.append((torch.stack([t['image'] for t in s]).to(dev), torch.stack([t['semantic_mask'] for t in s]).to(dev),
                    unl[2 * k].to(dev), unl[2 * k + 1].to(dev)))
    return out


def _train_run(dev, label_map, void=0.0, steps=2, graph=None, keep=None):
    """`steps` steps of the 5-class SimpleUNet at 64^2, batch 2, CowMix drawn on the device from a reset counter;
    graph None: train.train_step; True / False: train.run_step with the captured step on / off"""
    import cowmix
    import train
    from ssseg import arena, optim
    student, teacher, _, _ = _small_pair(NC, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    if keep is not None:
        keep.extend([student, teacher])      # the trainer keys its per-model step counts on id()
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    cfg = {'train': _tcfg('softmax', loss=_loss(label_map), ignore_label=255, print_freq=10 ** 9)}
    data = _batches(_dataset(label_map, void), steps, dev)
    assert cowmix.NOISE_SOURCE == 'device'
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    # a fresh model may get the id() of a freed one: its step count starts at 0 (two eager tuning steps first)
    train._OVERLAP['seen'].pop(train._step_key(student, teacher, data[0][0], data[0][2]), None)
    student.train()
    opt.zero_grad()
    if graph is None:
        out = [train.train_step(student, teacher, opt, *data[k], 26, k, cfg) for k in range(steps)]
        caps = 0
    else:
        was, cap0 = train._GRAPH['on'], train._GRAPH['captures']
        train._GRAPH['on'] = graph
        try:
            out = [train.run_step(student, teacher, opt, *data[k], 26, k, cfg) for k in range(steps)]
            torch.cuda.synchronize()
        finally:
            train._GRAPH['on'] = was
            train.release_graphs()
        caps = train._GRAPH['captures'] - cap0
    torch.cuda.synchronize()
    state = {**{'s.' + k: v.detach().clone() for k, v in student.state_dict().items()},
             **{'t.' + k: v.detach().clone() for k, v in teacher.state_dict().items()}}
    return [tuple(float(t) for t in o) for o in out], state, caps, data


def test_train_step_label_map_against_one_hot(hip_device, fp32_compute):
    dense, _, _, dd = _train_run(hip_device, False)
    sparse, _, _, ds = _train_run(hip_device, True)
    void, _, _, dv = _train_run(hip_device, True, void=0.25)
    print('one-hot', dense, 'label map', sparse, 'label map, a quarter void', void)
    assert dd[0][1].dim() == 4 and ds[0][1].dtype == torch.uint8 and tuple(ds[0][1].shape) == (2, 64, 64)
    assert torch.equal(dd[1][1].argmax(1), ds[1][1].long()) and torch.equal(dd[1][0], ds[1][0])
    share = float((dv[1][1] == 255).float().mean())
    assert 0.15 < share < 0.35 and not (ds[1][1] == 255).any()
    for a, b in zip(dense, sparse):
        assert _close(b[0], a[0], LOSS_TOL), (a, b)            # the classification loss of every step, step 1 included
    assert all(np.isfinite(l).all() for l in void)
    assert all(v[0] != s[0] for v, s in zip(void, sparse))


def test_validate_on_label_maps(hip_device, fp32_compute):
    import multiclass_ref as MR
    import train
    student = _small_pair(NC, hip_device)[0]

    def run(label_map, void=0.0):
        spy = _Spy(student)
        loader = torch.utils.data.DataLoader(_dataset(label_map, void, length=6, seed=4), batch_size=2)
        cfg = {'train': _tcfg('softmax', loss=_loss(label_map), ignore_label=255)}
        loss, metric = train.validate(spy, loader, 0, 0, None, cfg, hip_device)
        return float(loss), float(metric), train._VALIDATE['miou'], list(train._VALIDATE['class_ious']), spy, loader
    dense, sparse, void = run(False), run(True), run(True, 0.25)
    print('one-hot', dense[:4], 'label map', sparse[:4], 'a quarter void', void[:4])
    assert _close(sparse[0], dense[0], LOSS_TOL)
    assert sparse[1] == dense[1] and sparse[2] == dense[2] and sparse[3] == dense[3]
    # with void pixels: the host confusion matrix over the valid pixels only
    total, dices, nvoid = None, [], 0
    for logits, sample in zip([t.cpu() for t in void[4].seen], void[5]):
        lab = sample['semantic_mask']
        assert lab.dtype == torch.uint8 and lab.dim() == 3
        nvoid += int((lab == 255).sum())
        m = MR.seg_metrics(logits, lab.long(), ignore=255, total=total)
        pred = MR.predictions(logits, lab.shape[-2:])[1]
        assert torch.equal(m['conf'], R.confusion(pred, lab, NC, 255))
        total = m['conf'] if total is None else total + m['conf']
        dices.append(m['dice_mean'])
    assert nvoid > 0 and int(total.sum()) == 6 * 64 * 64 - nvoid
    assert np.allclose(void[1], np.mean(dices), rtol=1e-6, atol=0)
    assert np.allclose(void[2], 100 * m['miou'], rtol=1e-6, atol=0)
    assert np.allclose(void[3], 100 * m['ious'], rtol=1e-6, atol=0)
    assert void[2] != sparse[2] and np.isfinite(void[0])


def test_label_map_step_replays_a_captured_graph(hip_device, fp32_compute):
    keep = []
    l_e, s_e, caps_e, _ = _train_run(hip_device, True, void=0.25, steps=6, graph=False, keep=keep)
    l_g, s_g, caps_g, _ = _train_run(hip_device, True, void=0.25, steps=6, graph=True, keep=keep)
    print('eager', l_e, 'graph', l_g, 'captures', caps_g)
    assert caps_e == 0 and caps_g >= 1
    assert l_e == l_g and all(np.isfinite(l).all() for l in l_e)
    for k in s_e:
        assert torch.equal(s_e[k], s_g[k]), k
