"""GPU: the self-adaptive per-class confidence thresholds (ssseg_adaptive_thr_update, csrc/adaptive_thr.hip), the
pseudo-label cross-entropy with a threshold vector (ssseg_consistency_ce_cls_fwd / _bwd, csrc/multiclass.hip), both
through ops.AdaptiveThreshold / ops.consistency_loss_ce, and the training step that selects them with
train['confidence_threshold_mode'] = 'adaptive', against the fp64 restatement of tests/adaptive_thr_ref.py.

Bounds: the statistics of designed teachers (p exactly 1 / C, 1 or 0) are exact (torch.equal); everything else is under
the project's loss bounds (imported from test_hip_losses_ext.py): loss and statistics rtol 2e-5
atol 1e-7; gradient rtol 2e-4 atol 2e-8 at every element, exactly 0.0 wherever the fp64 gradient is 0; the step against
the oracle under the rules of tests/parity.py.  Where a mask is compared, every pixel's fp64 confidence is at least 1e-3
from its own threshold (asserted first: a condition on the inputs).  The kernels' own thresholds: less than a wave, the
256-pixel tile (17 * 31 = 527 pixels per sample), the channel buckets 2, 4, 8, 16, 32, 64 and the 8-channel chunks
(C = 8, 9, 16, 17, 32, 33 sit on both sides), more tiles than workgroups and more partial rows than final-block threads
(S_GRID).  Every test prints its figures before it asserts.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adaptive_thr_ref as A
import exact_losses as E
import mixmask_ref as MM
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL
from test_multiclass import _maxabs, _small_pair, _step_data, _tcfg, close, fp32_compute  # noqa: F401
from test_pseudo_ce import weight_maps

pytestmark = pytest.mark.gpu

C_LIST = [1, 2, 3, 4, 5, 8, 9, 16, 17, 19, 32, 33, 64]
WEIGHTINGS = ('pixel', 'batch')
S_GRID = tuple(E.S_GRID)


def dev_state(sat):
    C = sat.thr.numel()
    s = sat.state.cpu()
    return {'tau': s[0], 'ptilde': s[1:C + 1], 'steps': int(s[C + 1]), 'm': s[C + 2], 'q': s[C + 3:2 * C + 3],
            'thr': sat.thr.cpu()}


def alternating_thr(C):
    """0.6 for the even classes, 0.9 for the odd ones"""
    return torch.tensor([0.6, 0.9] * 32)[:C].contiguous()


def device_ce(s, t, thr, w, weighting, dev, gout=1.0):
    """-> (loss, cm mean, gradient of gout * loss) as numpy; thr a float or a [C] tensor"""
    from ssseg import ops
    x = s.to(dev).requires_grad_(True)
    thr = thr.to(dev) if isinstance(thr, torch.Tensor) else thr
    loss, cm = ops.consistency_loss_ce(x, t.to(dev), thr, None if w is None else w.to(dev), weighting)
    assert not cm.requires_grad
    (loss * gout).backward()
    return loss.detach().cpu().numpy(), cm.detach().cpu().numpy(), x.grad.cpu().numpy()


# ---- 1. the statistics, exact ----------------------------------------------------------------------------------------
def exact_teacher(shape, seed):
    """every pixel is an all-equal row (p = 1 / C exactly for C a power of two) or has one class at +1e4 over zeros
    (p exactly 1 and 0: expf(-1e4) is 0)"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    flat = torch.randint(-3, 4, (B, 1, H, W), generator=g).float().repeat(1, C, 1, 1)
    spike = torch.zeros(B, C, H, W).scatter_(1, torch.randint(0, C, (B, 1, H, W), generator=g), 1e4)
    return torch.where(torch.rand(B, 1, H, W, generator=g) < 0.5, spike, flat).contiguous()


@pytest.mark.parametrize('shape', [(2, 4, 7, 9)] + [(2, C, 17, 31) for C in (1, 2, 4, 8, 16, 32, 64)] + [S_GRID],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_statistics_exact(hip_device, shape):
    """a dropped tile, a double-counted tail or a wrong divisor fails exactly"""
    from ssseg import ops
    assert S_GRID == (3, 2, 1, 349_623) and S_GRID[0] * ((S_GRID[3] + 255) // 256) == 4098
    C = shape[1]
    sat, ref = ops.AdaptiveThreshold(0.5), A.sat_init(C)
    for k in range(3):
        t = exact_teacher(shape, 10 + k)
        thr = sat.update(t.to(hip_device))
        want, m, q = A.sat_update(ref, t, 0.5)
        got = dev_state(sat)
        print(f'{shape} step {k}: tau {float(got["tau"])!r} fp64 {float(ref["tau"])!r} m {float(got["m"])!r} '
              f'{float(m)!r} thr {got["thr"][:4].tolist()} {want[:4].tolist()}')
        assert thr is sat.thr and thr.dtype == torch.float32 and tuple(thr.shape) == (C,)
        assert torch.equal(got['m'], m) and torch.equal(got['q'], q)
        assert torch.equal(got['tau'], ref['tau']) and torch.equal(got['ptilde'], ref['ptilde'])
        assert got['steps'] == k + 1 == ref['steps'] and torch.equal(got['thr'], want)
    assert C == 1 or float(got['tau']) not in (1.0 / C, 1.0)     # both kinds of pixel were there


# ---- 2. the statistics, random ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, C, 17, 31) for C in C_LIST] + [S_GRID], ids=lambda s: 'x'.join(map(str, s)))
def test_statistics_random(hip_device, shape):
    from ssseg import ops
    C = shape[1]
    ts = [torch.randn(*shape, generator=torch.Generator().manual_seed(30 + C + k)) * 4 for k in range(3)]
    td = [t.to(hip_device) for t in ts]
    for momentum in (0.0, 0.5, 0.999):
        sat, ref = ops.AdaptiveThreshold(momentum), A.sat_init(C)
        first = []
        for k in range(3):
            sat.update(td[k])
            want, m, q = A.sat_update(ref, ts[k], momentum)
            got = dev_state(sat)
            first.append(got)
            rel = lambda a, b: float(((a.double() - b.double()).abs() / b.double().abs()).max())  # noqa: E731
            print(f'{shape} momentum {momentum} step {k}: m {float(got["m"])!r} fp64 {float(m)!r} | rel err q '
                  f'{rel(got["q"], q):.2e} tau {rel(got["tau"], ref["tau"]):.2e} ptilde '
                  f'{rel(got["ptilde"], ref["ptilde"]):.2e} thr {rel(got["thr"], want):.2e}')
            for name, a, b in (('m', got['m'], m), ('q', got['q'], q), ('tau', got['tau'], ref['tau']),
                               ('ptilde', got['ptilde'], ref['ptilde']), ('thr', got['thr'], want.double())):
                assert close(a.numpy(), b.numpy(), LOSS_TOL), name
            assert got['steps'] == k + 1
        if momentum == 0.0:     # no memory: the state is this batch's statistics
            assert torch.equal(got['tau'], got['m']) and torch.equal(got['ptilde'], got['q'])
        # a second run from reset() is bit-identical, in the same storage
        ptrs = (sat.state.data_ptr(), sat.thr.data_ptr())
        sat.reset()
        zero = dev_state(sat)
        assert zero['steps'] == 0 and float(zero['tau']) == 1.0 / C and torch.equal(zero['ptilde'], A.sat_init(C)['ptilde'])
        assert torch.equal(zero['thr'], torch.full((C,), 1.0 / C, dtype=torch.float64).float())
        for k in range(3):
            sat.update(td[k])
            again = dev_state(sat)
            for key in ('tau', 'ptilde', 'm', 'q', 'thr'):
                assert torch.equal(again[key], first[k][key]), key
        assert ptrs == (sat.state.data_ptr(), sat.thr.data_ptr())


# ---- 3. the cross-entropy with a threshold vector --------------------------------------------------------------------
def check_ce(name, s, t, thr_c, dev, w, weighting, gout, ref=A.pseudo_ce_grad):
    l64, cm64, scm64, g64 = ref(s, t, thr_c, w, weighting, gout)
    loss, cm, grad = device_ce(s, t, thr_c, w, weighting, dev, gout)
    bad = ~np.isclose(grad, g64, equal_nan=True, **GRAD_TOL)
    print(f'{name} {tuple(s.shape)} {weighting}: loss dev {loss!r} fp64 {l64!r} rel {abs(loss - l64) / abs(l64 + 1e-300):.2e}'
          f' | cm {cm!r} fp64 {cm64!r} | grad dev-fp64 {_maxabs(grad - g64):.3e} of {_maxabs(g64):.3e}, '
          f'{int(bad.sum())} of {bad.size} out of bound')
    assert loss.dtype == np.float32 and grad.shape == g64.shape
    assert close(loss, l64, LOSS_TOL)
    assert not bad.any()
    assert np.all(grad[g64 == 0] == 0)
    if w is None:   # the fraction is the count, exactly
        assert cm == np.float32(float(scm64) / s[:, 0].numel())
    else:
        assert close(cm, cm64, LOSS_TOL)
    return loss, cm, grad, (l64, g64)


def check_shape(shape, seed, dev, maps=('none', 'binary', 'fractional')):
    C = shape[1]
    t, thr_c = A.tiered_teacher(shape, seed), alternating_thr(C)
    s = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1000)).contiguous()
    dist, on = A.min_distance(t, thr_c), A.confident(t, thr_c)
    print(f'{shape}: distance {dist:.3e} confident {float(on.float().mean()):.3f}')
    assert dist >= 1e-3
    if C > 1:
        assert 0 < int(on.sum()) < on.numel()
        # the vector decides otherwise than either of its two values would as a scalar
        conf = A.confidence(t)[0]
        assert int((on != (conf > 0.6)).sum()) > 0 and int((on != (conf > 0.9)).sum()) > 0
    ws = weight_maps(shape, seed)
    gout = on.numel() / 16.0    # the gradient O(1 / 16) per pixel: the relative bound is the one that binds
    for weighting in WEIGHTINGS:
        got = {k: check_ce(f'w={k}', s, t, thr_c, dev, ws[k], weighting, gout) for k in maps}
        for k in ('binary', 'fractional'):
            if k in got:
                assert np.all(got[k][2].transpose(0, 2, 3, 1)[(ws[k] == 0).numpy()] == 0)
        if weighting == 'pixel':
            assert np.all(got['none'][2].transpose(0, 2, 3, 1)[(~on).numpy()] == 0)


def test_ce_vector_less_than_a_wave(hip_device):
    check_shape((2, 3, 7, 9), 3, hip_device)


@pytest.mark.parametrize('C', C_LIST)
def test_ce_vector_channel_buckets_and_tiles(hip_device, C):
    check_shape((2, C, 17, 31), 40 + C, hip_device)


def test_ce_vector_more_tiles_than_workgroups(hip_device):
    check_shape(S_GRID, 7, hip_device, maps=('none', 'fractional'))


# ---- 4. one value in every class is the scalar kernel, bit for bit ---------------------------------------------------
@pytest.mark.parametrize('C', [3, 8, 19, 64])
def test_vector_of_one_value_is_the_scalar_bitwise(hip_device, C):
    from ssseg import native as N
    shape, theta = (2, C, 17, 31), 0.6
    B, HW = 2, 17 * 31
    t = A.tiered_teacher(shape, 60 + C).to(hip_device)
    s = torch.randn(*shape, generator=torch.Generator().manual_seed(C)).to(hip_device)
    w = weight_maps(shape, C)['fractional'].to(hip_device)
    thr_c = torch.full((C,), theta, device=hip_device)
    gout = torch.tensor([B * HW / 16.0], device=hip_device)
    nb = N.lib().ssseg_consistency_ce_workspace_bytes(B * HW)
    p = N.dev_ptr
    for weighting in (0, 1):
        for wt in (None, w):
            res = []
            for cls in (False, True):
                out, ws, gs = torch.zeros(4, device=hip_device), N.workspace(nb, hip_device), torch.zeros_like(s)
                th = p(thr_c) if cls else theta
                sfx = '_cls' if cls else ''
                N.call(f'ssseg_consistency_ce{sfx}_fwd', p(s), p(t), p(wt), B, C, HW, th, weighting, p(out), p(ws), nb,
                       N.stream())
                N.call(f'ssseg_consistency_ce{sfx}_bwd', p(s), p(t), p(wt), B, C, HW, th, weighting, p(out), p(gout),
                       p(gs), N.stream())
                res.append((out.cpu(), gs.cpu()))
            print(f'C={C} weighting {weighting} w {wt is not None}: out4 {res[0][0].tolist()} {res[1][0].tolist()}')
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
            assert 0 < float(res[0][0][2]) < float(res[0][0][3]) and float(res[0][1].abs().sum()) > 0
    # and through the op: the loss and the gradient
    for weighting in WEIGHTINGS:
        a = device_ce(s.cpu(), t.cpu(), theta, None, weighting, hip_device, 33.0)
        b = device_ce(s.cpu(), t.cpu(), thr_c, None, weighting, hip_device, 33.0)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---- 5. the comparison can fail --------------------------------------------------------------------------------------
def test_comparison_can_fail(hip_device):
    """the scalar tau in the vector's place, the vector reversed, the threshold read at the student's argmax and a
    negated gradient all break the comparison of section 3"""
    shape = (2, 3, 17, 31)
    t = A.tiered_teacher(shape, A.TIER_SEED)
    s = torch.randn(*shape, generator=torch.Generator().manual_seed(9)).contiguous()
    state = A.sat_init(3)
    thr_c, _, _ = A.sat_update(state, t, 0.0)
    tau = torch.full((3,), float(state['tau']))
    ys = torch.argmax(s, 1)
    print('thr', thr_c.tolist(), 'tau', float(state['tau']))
    on = A.confident(t, thr_c)
    conf = A.confidence(t)[0]
    others = {'tau': conf > tau[0].double(), 'reversed': A.confident(t, thr_c.flip(0)),
              'student label': conf > thr_c.double()[ys]}
    for k, v in others.items():
        print(k, 'differs in', int((v != on).sum()), 'pixels')
        assert int((v != on).sum()) > 10
    assert min(A.min_distance(t, thr_c), A.min_distance(t, thr_c.flip(0)), A.min_distance(t, tau)) >= 1e-3
    gout = on.numel() / 16.0
    loss, _, grad, (l64, g64) = check_ce('C=3', s, t, thr_c, hip_device, None, 'pixel', gout)
    assert not close(-grad, g64, GRAD_TOL) and not close(0 * grad, g64, GRAD_TOL)
    mutants = {'tau': lambda s, t, c, w, wt, g: A.pseudo_ce_grad(s, t, tau, w, wt, g),
               'reversed': lambda s, t, c, w, wt, g: A.pseudo_ce_grad(s, t, c.flip(0), w, wt, g),
               'student label': lambda s, t, c, w, wt, g: A.pseudo_ce_grad(s, t, c, w, wt, g, label=ys),
               'negated': lambda s, t, c, w, wt, g: tuple(-x if i == 3 else x for i, x in
                                                           enumerate(A.pseudo_ce_grad(s, t, c, w, wt, g)))}
    for name, ref in mutants.items():
        with pytest.raises(AssertionError):
            check_ce(name, s, t, thr_c, hip_device, None, 'pixel', gout, ref=ref)


# ---- 6. end to end through the op ------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 5, 19])
@pytest.mark.parametrize('momentum', [0.0, 0.5])
def test_update_then_loss_masks_equal_the_restatement(hip_device, C, momentum):
    from ssseg import ops
    shape = (2, C, 17, 31)
    sat, ref = ops.AdaptiveThreshold(momentum), A.sat_init(C)
    for k in range(3):
        t = A.tiered_teacher(shape, A.TIER_SEED + k)
        s = torch.randn(*shape, generator=torch.Generator().manual_seed(k)).to(hip_device).requires_grad_(True)
        want, _, _ = A.sat_update(ref, t, momentum)
        dist, on = A.min_distance(t, want), A.confident(t, want)
        td = t.to(hip_device)
        loss, cm = ops.consistency_loss_ce(s, td, sat.update(td), None, 'pixel')
        loss.backward()
        mask = (s.grad != 0).any(1).cpu()
        l64, cm64, _, _ = A.pseudo_ce_grad(s.detach().cpu(), t, want)
        print(f'C={C} momentum {momentum} step {k}: distance {dist:.3e} confident {float(on.float().mean()):.3f} '
              f'mask differs in {int((mask != on).sum())} | thr dev {sat.thr.cpu()[:3].tolist()} fp64 '
              f'{want[:3].tolist()} | loss {float(loss.detach())!r} fp64 {l64!r}')
        assert dist >= 1e-3
        assert close(sat.thr.cpu().numpy(), want.numpy(), LOSS_TOL)
        assert torch.equal(mask, on) and float(cm) == np.float32(float(on.sum()) / on.numel())
        assert close(float(loss.detach()), l64, LOSS_TOL)
        if momentum == 0.0:
            assert 0 < int(on.sum()) < on.numel()


# ---- 7. edge semantics -----------------------------------------------------------------------------------------------
def test_one_class(hip_device):
    """C = 1: p = 1 everywhere, tau and thr stay 1.0, conf = 1 is not > 1: nothing is confident, the loss is 0.0"""
    from ssseg import ops
    sat = ops.AdaptiveThreshold(0.5)
    for k in range(3):
        t = torch.randn(2, 1, 17, 31, generator=torch.Generator().manual_seed(k)) * 4
        thr = sat.update(t.to(hip_device))
        got = dev_state(sat)
        assert float(got['tau']) == 1.0 and float(got['ptilde'][0]) == 1.0 and float(thr[0]) == 1.0
        s = torch.randn(2, 1, 17, 31)
        loss, cm, grad = device_ce(s, t, sat.thr, None, 'pixel', hip_device)
        print(f'step {k}: thr {float(thr[0])!r} loss {loss!r} cm {cm!r}')
        assert loss == 0.0 and not np.signbit(loss) and cm == 0.0 and np.all(grad == 0)


def test_argmax_rule_ties_and_nan_with_the_vector(hip_device):
    """test_pseudo_ce.py's rows; the thresholds make the label that reads them visible: every row's own class (the
    first maximum, the first NaN) has 0.3, every other class 0.999, which no row's confidence passes"""
    nan = float('nan')
    rows = [[1.0, 3.0, 0.0, 3.0, 2.0],        # two-way tie: the first maximum, 1
            [2.0, 0.0, 2.0, -1.0, 2.0],       # three-way tie: 0
            [0.0, 4.0, 4.0, 4.0, 1.0],        # three-way tie inside: 1
            [0.0, 0.0, 0.0, 0.0, 0.0],        # all equal: 0
            [1.0, 2.0, nan, 9.0, 3.0],        # NaN counts as the maximum, also before a larger value: 2
            [1.0, nan, 5.0, nan, 0.0],        # the first NaN: 1
            [nan, 7.0, 1.0, 2.0, 3.0],        # NaN in channel 0: 0
            [-1.0, -2.0, -3.0, -0.5, -0.5]]   # a tie in the last two: 3
    want = torch.tensor([1, 0, 1, 0, 2, 1, 0, 3])
    for C in (5, 9):    # one chunk, and the same rows spread over two 8-channel chunks (channel c -> 2c)
        t = torch.full((2, C, 2, 4), -50.0)
        src = torch.tensor(rows).t().reshape(5, 2, 4)
        step = 1 if C == 5 else 2
        t[0, ::step] = src
        t[1, ::step] = src.flip(2)
        label = torch.stack([want.view(2, 4), want.view(2, 4).flip(1)]) * step
        assert torch.equal(torch.argmax(t, 1), label)
        s = torch.randn(2, C, 2, 4, generator=torch.Generator().manual_seed(C))
        onehot = F.one_hot(label, C).permute(0, 3, 1, 2).bool()
        # the labels in use are 0, 1, 2, 3 (times step); class 4 (times step) is never a label.  Classes 0 and 1 get
        # 0.3, classes 2, 3 and the rest 0.999: the rows labelled 2 (NaN) and 3 (the last-two tie, confidence 0.33) are
        # unconfident only because THEIR class's entry is read, and the ties at 1 / 0 are confident only because the
        # FIRST maximum's entry is read (the later maxima, classes 2 and 3, have 0.999)
        thr_c = torch.full((C,), 0.999)
        thr_c[0], thr_c[step] = 0.3, 0.3
        conf = torch.softmax(t.double(), 1).amax(1)
        on = conf > thr_c.double()[label]           # NaN rows: False
        finite = ~torch.isnan(conf)
        assert float((conf - thr_c.double()[label])[finite].abs().min()) >= 1e-3
        assert 0 < int(on.sum()) < on.numel() and on[label == 3 * step].sum() == 0 and on[0, 0, 0] and on[0, 0, 1]
        assert int((on != (conf > 0.3)).sum()) > 0          # the scalar 0.3 would decide otherwise (the last-two tie)
        # 'batch': every pixel has a gradient, negative only at the label; the loss picks s[y]
        loss, cm, grad = device_ce(s, t, thr_c, None, 'batch', hip_device, gout=16.0)
        l64, cm64, _, g64 = A.pseudo_ce_grad(s, t, thr_c, None, 'batch', gout=16.0)
        print(f'C={C}: loss {loss!r} fp64 {l64!r} cm {cm!r} fp64 {cm64!r}')
        assert torch.equal(torch.from_numpy(grad < 0), onehot)
        assert np.isfinite(grad).all() and close(loss, l64, LOSS_TOL) and close(grad, g64, GRAD_TOL)
        assert cm == np.float32(cm64) == np.float32(float(on.sum()) / on.numel())
        # 'pixel': exact zeros where the pixel is not confident, the label's sign pattern elsewhere
        _, _, grad = device_ce(s, t, thr_c, None, 'pixel', hip_device, gout=16.0)
        assert torch.equal(torch.from_numpy(grad < 0), onehot & on.unsqueeze(1))
        assert np.all(grad.transpose(0, 2, 3, 1)[(~on).numpy()] == 0)


def test_unconfident_pixels_are_selected_out(hip_device):
    for C in (3, 19):
        shape = (2, C, 17, 31)
        t, thr_c = A.tiered_teacher(shape, 70 + C), alternating_thr(C)
        on = A.confident(t, thr_c)
        assert A.min_distance(t, thr_c) >= 1e-3 and 0 < int(on.sum()) < on.numel()
        g = torch.Generator().manual_seed(C)
        s = torch.randn(*shape, generator=g)
        wild = torch.tensor([1e4, -1e4, float('nan')])[torch.randint(0, 3, s.shape, generator=g)]
        s_wild = torch.where(on.unsqueeze(1), s, wild)
        assert int(torch.isnan(s_wild).sum()) > 50
        gout = on.numel() / 16.0
        loss, cm, grad = device_ce(s_wild, t, thr_c, None, 'pixel', hip_device, gout)
        l64 = A.pseudo_ce(s_wild.double(), t.double(), thr_c)[0].numpy()
        # (the gradient's yardstick: the fp64 gradient on the student with the selected-out pixels zeroed -- autograd
        # through torch.where gives 0 * NaN there -- which is the same loss)
        l64b, _, _, g64 = A.pseudo_ce_grad(torch.where(on.unsqueeze(1), s, torch.zeros(())), t, thr_c, None, 'pixel', gout)
        print(f'C={C}: wild student loss dev {loss!r} fp64 {l64!r} (tame {l64b!r}); grad dev-fp64 {_maxabs(grad - g64):.3e}')
        assert l64 == l64b and np.isfinite(loss) and close(loss, l64, LOSS_TOL)
        assert close(grad, g64, GRAD_TOL) and np.all(grad.transpose(0, 2, 3, 1)[(~on).numpy()] == 0)
        # no class lets a pixel through: exactly 0.0 and an all-zero gradient
        loss, cm, grad = device_ce(s_wild, t, torch.ones(C), None, 'pixel', hip_device, gout)
        assert loss == 0.0 and not np.signbit(loss) and cm == 0.0 and np.all(grad == 0)


def test_refusals_before_any_launch(hip_device):
    from ssseg import native as N
    from ssseg import ops
    x = torch.zeros(2, 3, 7, 9, device=hip_device)
    with pytest.raises(ValueError, match='one per class'):
        ops.consistency_loss_ce(x, x, torch.zeros(4, device=hip_device))
    with pytest.raises(ValueError, match='threshold vector is on'):
        ops.consistency_loss_ce(x, x, torch.zeros(3))
    sat = ops.AdaptiveThreshold(0.5)
    sat.update(x)
    with pytest.raises(ValueError, match='3 classes'):
        sat.update(torch.zeros(2, 5, 7, 9, device=hip_device))
    with pytest.raises(ValueError, match='HIP device tensor'):
        sat.update(x.cpu())
    with pytest.raises(ValueError, match='5 classes'):
        sat.load_state_dict({'tau': 0.2, 'ptilde': [0.2] * 5, 'steps': 0})
    before = dev_state(sat)
    # the entry point itself, with device pointers: a bad momentum, 65 classes, a short workspace
    lib, p = N.lib(), N.dev_ptr
    ws = torch.zeros(8 * 1024 * 4, dtype=torch.uint8, device=hip_device)
    assert lib.ssseg_adaptive_thr_update(p(x), 2, 3, 63, 1.0, p(sat.state), p(sat.thr), p(ws), ws.numel(), None) == -1
    assert lib.ssseg_adaptive_thr_update(p(x), 2, 65, 63, 0.5, p(sat.state), p(sat.thr), p(ws), ws.numel(), None) == -1
    assert lib.ssseg_adaptive_thr_update(p(x), 2, 3, 63, 0.5, p(sat.state), p(sat.thr), p(ws), ws.numel() - 8, None) == -3
    assert lib.ssseg_consistency_ce_cls_fwd(p(x), p(x), None, 2, 3, 63, None, 0, p(ws), p(ws), ws.numel(), None) == -1
    torch.cuda.synchronize()
    after = dev_state(sat)
    assert all(torch.equal(torch.as_tensor(before[k]), torch.as_tensor(after[k])) for k in before)
    assert float(ws.sum()) == 0.0


# ---- 8. the training step --------------------------------------------------------------------------------------------
STEP_MOMENTUM = 0.5


def test_step_vs_oracle_cutmix_pixel(hip_device, fp32_compute, monkeypatch):  # noqa: F811
    """three semi-supervised steps of a 5-class SimpleUNet at 64^2, batch 2, epoch 26, CutMix masks from host-fixed
    draws, 'ce' / 'pixel' with adaptive thresholds of momentum 0.5, against the oracle's train_epoch with its
    consistency_loss swapped for a stateful restatement (the recorded masks handed to the oracle in order, as
    test_mixmask.py does).  fp64 oracle, momentum 0.5, these seeds: confident fractions 0.905, 0.822, 0.750 (asserted
    inside (0.05, 0.95): a condition on the input), tau 0.363, 0.454, 0.486, thresholds from 0.13 to 0.49 at step 2.
    The thresholds and tau are held to the 1e-3 of tests/parity.py against the fp64 oracle's."""
    import cowmix
    import mixmasks
    import train
    from oracle import train_ref
    from parity import check_losses, tensor_outliers
    from ssseg import arena, optim
    C, steps = 5, 3
    student, teacher, ref_s, ref_t = _small_pair(C, hip_device)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    imgs, masks, unl = _step_data(C, steps)
    tc = _tcfg('softmax', mix_mask='cutmix', consistency_loss='ce', consistency_ce_weighting='pixel',
               confidence_threshold_mode='adaptive', confidence_threshold_momentum=STEP_MOMENTUM)
    params = MM.DESIGNED[[0, 7]]
    seen = []
    real = mixmasks.generate_cutmix_masks_like

    def recording(example, *a, **kw):
        m = real(example, *a, **kw)
        seen.append(m.detach().float().cpu())
        return m
    monkeypatch.setattr(mixmasks, 'generate_cutmix_masks_like', recording)
    monkeypatch.setattr(cowmix, 'generate_cowmix_masks_like', None)        # the step must not take the CowMix path
    mixmasks.set_draws(params=params)
    try:
        student.train()
        opt.zero_grad()
        logs, taus = [], []
        for k in range(steps):
            c, u, cm = train.train_step(student, teacher, opt, imgs[k].to(hip_device), masks[k].to(hip_device),
                                        unl[2 * k].to(hip_device), unl[2 * k + 1].to(hip_device), 26, k, {'train': tc})
            logs.append((float(c), float(u), float(cm)))
            taus.append(dev_state(tc['confidence_threshold_state']))
            print(f'step {k}: sup {float(c)!r} unsup {float(u)!r} cm {float(cm)!r} tau {float(taus[-1]["tau"])!r} thr '
                  f'{taus[-1]["thr"].tolist()}')
            if k == 0:
                ghip = {n: p.grad.detach().cpu().double().numpy().copy() for n, p in student.named_parameters()}
    finally:
        mixmasks.set_draws()
    ref_mask, _ = MM.cutmix(params, 64, 64, tc['mask_proportion_range'])
    assert len(seen) == steps and all(torch.equal(m, ref_mask) for m in seen) and 0 < float(ref_mask.mean()) < 1

    def oracle(dt, pert=0.0):
        s, t = copy.deepcopy(ref_s).to(dt), copy.deepcopy(ref_t).to(dt)
        o = torch.optim.SGD(s.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
        x, u = imgs.to(dt), unl.to(dt)
        if pert:   # the step's own sensitivity (tests/parity.py): inputs moved by ~fp32 rounding
            gp = torch.Generator().manual_seed(99)
            x = x * (1 + pert * torch.randn(x.shape, generator=gp, dtype=dt))
            u = u * (1 + pert * torch.randn(u.shape, generator=gp, dtype=dt))
        state, states = A.sat_init(C), []

        def stateful(sp, tp, thr):
            thr_c, _, _ = A.sat_update(state, tp, STEP_MOMENTUM)
            states.append((float(state['tau']), thr_c.clone()))
            return A.pseudo_ce(sp, tp, thr_c, None, 'pixel')[:2]
        monkeypatch.setattr(train_ref, 'consistency_loss', stateful)
        recorded = iter(seen)
        monkeypatch.setattr(train_ref, 'cowmix_mask_like', lambda ex, *a, **kw: next(recorded).to(ex.dtype))
        g0 = {}

        def grab(step, rec):   # step 0 runs no optimizer step: its gradients are still in .grad
            if step == 0:
                g0.update({k: p.grad.detach().double().numpy().copy() for k, p in s.named_parameters()})
        lg = train_ref.train_epoch(s, t, o, list(zip(x, masks.to(dt))), iter(u), 26,
                                   train_ref.default_cfg(sigma_range=(2, 4), confidence_threshold=0.5), on_step=grab)
        return lg, states, g0
    r32, _, g32 = oracle(torch.float32)
    r64, st64, g64 = oracle(torch.float64)
    _, _, gp = oracle(torch.float64, pert=1e-6)
    print('oracle fp64:', r64, [(a, b.tolist()) for a, b in st64])
    assert all(0.05 < r['cm_mean'] < 0.95 and r['unsup_loss'] > 0 for r in r64)   # both kinds of pixel, the gate open
    assert float((st64[-1][1] - 1.0 / C).abs().max()) > 0.05                      # the thresholds have left 1 / C
    check_losses([l[:2] for l in logs], [(r['sup_loss'], r['unsup_loss']) for r in r32],
                 [(r['sup_loss'], r['unsup_loss']) for r in r64])
    for k in range(steps):   # the state: fp32 softmax statistics of fp32 teacher logits against the fp64 oracle's
        print(f'step {k}: tau dev {float(taus[k]["tau"])!r} fp64 {st64[k][0]!r} cm dev {logs[k][2]!r} fp64 '
              f'{r64[k]["cm_mean"]!r}')
        assert abs(float(taus[k]['tau']) - st64[k][0]) <= 1e-3 * st64[k][0]
        assert float((taus[k]['thr'].double() - st64[k][1].double()).abs().max()) <= 1e-3
    gfloor = 1e-3 * max(float(np.abs(v).max()) for v in g64.values())
    gbad = tensor_outliers(ghip, g32, g64, gp, floor=gfloor)
    print('step-0 gradient outliers:', gbad[:5])
    assert not gbad, gbad[:5]


# ---- 9. capture, defaults, checkpoint --------------------------------------------------------------------------------
def _steps(dev, tc, n_eager, n_graph=0, reload_after=None):
    """n_eager eager steps, then n_graph replays of one captured step; CowMix drawn on the device, its counter reset.
    reload_after: after that many steps the threshold state goes through state_dict() into a fresh object.
    -> (losses, the Philox counter, the final threshold state or None, (student, teacher, opt, data, cfg))"""
    import cowmix
    import train
    from ssseg import arena, ops, optim
    from ssseg.graph import StepGraph
    C = 5
    student, teacher, _, _ = _small_pair(C, dev)
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    n = n_eager + n_graph
    imgs, masks, unl = _step_data(C, n)
    data = [(imgs[k].to(dev), masks[k].to(dev), unl[2 * k].to(dev), unl[2 * k + 1].to(dev)) for k in range(n)]
    cfg = {'train': tc}
    assert cowmix.NOISE_SOURCE == 'device'
    for c in cowmix._DEVICE_RNG['ctr'].values():
        c.zero_()
    student.train()
    opt.zero_grad()
    out = []
    for k in range(n_eager):
        if reload_after is not None and k == reload_after:
            sd = tc['confidence_threshold_state'].state_dict()
            assert sd['steps'] == k and len(sd['ptilde']) == C and isinstance(sd['tau'], float)
            fresh = ops.AdaptiveThreshold(tc['confidence_threshold_momentum'])
            fresh.load_state_dict(sd)
            tc['confidence_threshold_state'] = fresh
        out.append(train.train_step(student, teacher, opt, *data[k], 26, k, cfg))
    if n_graph:
        assert train._graph_key(student, teacher, opt, *data[n_eager], 26, n_eager, cfg) is not None
        g = StepGraph(lambda i, m, a, b: train.train_step(student, teacher, opt, i, m, a, b, 26, n_eager, cfg),
                      *data[n_eager])
        for k in range(n_eager, n):
            out.append(tuple(t.clone() for t in g(*data[k])))
    torch.cuda.synchronize()
    ctr = int(cowmix._DEVICE_RNG['ctr'][dev.index if dev.index is not None else torch.cuda.current_device()])
    sat = tc.get('confidence_threshold_state')
    return ([tuple(float(t) for t in l) for l in out], ctr, dev_state(sat) if sat is not None else None,
            (student, teacher, opt, data, cfg))


def _adaptive_tc(**over):
    return _tcfg('softmax', consistency_loss='ce', confidence_threshold_mode='adaptive',
                 confidence_threshold_momentum=0.5, **over)


@pytest.mark.parametrize('weighting', WEIGHTINGS)
def test_adaptive_step_graph_replay_matches_eager_bitwise(hip_device, fp32_compute, weighting):  # noqa: F811
    import train
    eager, ctr_e, st_e, _ = _steps(hip_device, _adaptive_tc(consistency_ce_weighting=weighting), 5)
    graph, ctr_g, st_g, (student, teacher, opt, data, cfg) = _steps(
        hip_device, _adaptive_tc(consistency_ce_weighting=weighting), 2, 3)
    print('eager', eager, 'graph', graph, 'tau', float(st_e['tau']), float(st_g['tau']), 'thr', st_e['thr'].tolist())
    assert np.array_equal(np.array(eager), np.array(graph), equal_nan=True) and ctr_e == ctr_g
    assert all(np.isfinite(l).all() and l[1] > 0 and 0 < l[2] <= 1 for l in eager)
    assert st_e['steps'] == st_g['steps'] == 5          # every step, eager or replayed, updated the state
    for k in ('tau', 'ptilde', 'm', 'q', 'thr'):
        assert torch.equal(st_e[k], st_g[k]), k
    assert float((st_e['thr'] - 0.2).abs().max()) > 0.01      # and the thresholds have moved
    # a replay repeats its capture's choice: 'fixed', 'adaptive', another momentum and another state object each have a
    # key of their own
    tc = cfg['train']
    keys = {'adaptive': train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg)}
    tc['confidence_threshold_momentum'] = 0.9
    keys['momentum'] = train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg)
    tc['confidence_threshold_momentum'] = 0.5
    assert train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg) == keys['adaptive']
    tc['confidence_threshold_mode'] = 'fixed'
    keys['fixed'] = train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg)
    del tc['confidence_threshold_mode']
    assert train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg) == keys['fixed']
    tc['confidence_threshold_mode'] = 'adaptive'
    tc['confidence_threshold_state'] = type(tc['confidence_threshold_state'])(0.5)
    assert train._graph_key(student, teacher, opt, *data[0], 26, 5, cfg) is None   # no device state yet: an eager step
    assert all(k is not None for k in keys.values()) and len(set(keys.values())) == 3


def test_without_the_keys_is_the_fixed_ce_step_bitwise(hip_device, fp32_compute):  # noqa: F811
    none, ctr_n, st_n, _ = _steps(hip_device, _tcfg('softmax', consistency_loss='ce'), 3)
    fixed, ctr_f, st_f, _ = _steps(hip_device, _tcfg('softmax', consistency_loss='ce', confidence_threshold_mode='fixed',
                                                    confidence_threshold_momentum=0.5), 3)
    adap, ctr_a, st_a, _ = _steps(hip_device, _adaptive_tc(), 3)
    print('no key', none, 'fixed', fixed, 'adaptive', adap)
    assert np.array(none).tobytes() == np.array(fixed).tobytes() and ctr_n == ctr_f and ctr_n > 0
    assert st_n is None and st_f is None and st_a['steps'] == 3
    # another threshold on the same draws: the same supervised loss at step 0, another unsupervised loss
    assert adap[0][0] == none[0][0] and adap[0][1] != none[0][1] and ctr_a == ctr_n


def test_checkpoint_round_trip_on_the_device(hip_device, fp32_compute):  # noqa: F811
    whole, ctr_w, st_w, _ = _steps(hip_device, _adaptive_tc(), 3)
    resumed, ctr_r, st_r, _ = _steps(hip_device, _adaptive_tc(), 3, reload_after=2)
    print('uninterrupted', whole, 'reloaded after two steps', resumed)
    assert np.array(whole).tobytes() == np.array(resumed).tobytes() and ctr_w == ctr_r
    assert st_w['steps'] == st_r['steps'] == 3
    for k in ('tau', 'ptilde', 'thr'):
        assert torch.equal(st_w[k], st_r[k]), k
