"""Keeps tests/exact_aux.py honest without a GPU.  For every Tier A case of test_aux_exact.py: the fp64 reference
satisfies the exact-range condition in every compute mode (torch.equal against the kernels is legitimate), is
non-degenerate (the comparison can see a wrong read) and, for the designed BatchNorm statistics, has exactly the
moments the construction promises.  For every Tier B case with a ReLU: no pre-activation of the reference lies within
the bound of 0, so the reference's mask is the mask of every result inside the bound."""
import pytest
import torch
import torch.nn.functional as F

import exact as E
import exact_aux as A


def _range_all_modes(tensors, shift=0, fp32=()):
    for mode in E.MODES:
        E.check_exact_range(tensors, mode, shift, fp32)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
def _bn_cases(cases=A.BN_CASES):
    seen, out = set(), []
    for C, nhw in cases:
        for mode in E.MODES:
            c = A.chans(C, mode)
            if (c, nhw) not in seen:
                seen.add((c, nhw))
                out += [pytest.param(c, nhw, relu, res, id=f'{A.bn_id(c, nhw)}-relu{int(relu)}-res{int(res)}')
                        for relu, res in A.BN_FLAGS]
    return out


# (+ C = 10: the native 8-byte-chunk case)
@pytest.mark.parametrize('C,nhw,relu,residual', _bn_cases() + _bn_cases([(20, A.BN_MAP)])[:4])
def test_bn_train_is_exact_and_nondegenerate(C, nhw, relu, residual):
    ref = A.bn_train_reference(C, nhw, relu, residual)
    P = nhw[0] * nhw[1] * nhw[2]
    for mode in E.MODES:
        A.bn_train_check_range(ref, mode)
    # the designed statistics: mean = m, invstd = 1 / s, x_hat = r, exactly
    assert torch.equal(ref['mean'], ref['m']) and torch.equal(ref['invstd'], 1.0 / ref['s'])
    assert set(ref['s'].tolist()) <= {1.0, 2.0, 4.0} and set(ref['gamma'].tolist()) <= {0.5, 1.0, 2.0}
    r, live = ref['r'], ref['live']
    full = lambda v: torch.full((C,), float(v), dtype=torch.float64)  # noqa: E731
    assert torch.equal(r.sum(1), full(0)) and torch.equal((r * r).sum(1), full(P))
    # the live set is the mask of the reference, with the promised moments
    assert torch.equal(A._cp(ref['z']) > 0, live) if relu else bool(live.all())
    L, s1, s2 = live.sum(1).double(), (r * live).sum(1), (r * r * live).sum(1)
    want = {(False, False): (P, 0, P), (False, True): (P, 0, P), (True, False): (5 * P / 16, 6 * P / 16, 8 * P / 16),
            (True, True): (P / 2, 0, P / 2)}[(relu, residual)]
    for got, w in zip((L, s1, s2), want):
        assert torch.equal(got, full(w))
    ml, mr = L / P, s1 / P
    assert torch.equal(ref['mdy'], ref['a'] * ml + ref['b'] * mr)
    assert torch.equal(ref['mdyx'], ref['a'] * mr + ref['b'] * (s2 / P))
    # non-degeneracy (a ReLU closes part of y and of the residual gradient by construction: 5/16 or 1/2 stay open)
    A.nondegenerate(ref['y'], 'y', 0.3 if relu else 0.5)
    A.nondegenerate(ref['dx'], 'dx', 0.5)
    if residual:
        A.nondegenerate(ref['dres'], 'dres', 0.3 if relu else 0.5)
    if C > 1:
        assert len(set(ref['dgamma'].tolist())) > 1 and len(set(ref['dbeta'].tolist())) > 1
    # the written-out backward is the gradient of the written-out forward (fp64 autograd, eps = 0)
    if P <= 4096:
        x = A._cp(ref['x']).clone().requires_grad_(True)
        gm, bt = ref['gamma'].clone().requires_grad_(True), ref['beta'].clone().requires_grad_(True)
        res = A._cp(ref['res']).clone().requires_grad_(True) if residual else None
        xh = (x - x.mean(1, keepdim=True)) / x.var(1, unbiased=False, keepdim=True).sqrt()
        z = gm[:, None] * xh + bt[:, None] + (res if residual else 0.0)
        (F.relu(z) if relu else z).backward(A._cp(ref['gy']))
        grads = (('dx', x.grad), ('dgamma', gm.grad), ('dbeta', bt.grad)) + ((('dres', res.grad),) if residual else ())
        for name, got in grads:
            want_ = A._cp(ref[name]) if ref[name].dim() == 4 else ref[name]
            assert float((got - want_).abs().max()) <= 1e-11, name


@pytest.mark.parametrize('C,nhw,relu,residual', _bn_cases(A.BN_EVAL_CASES))
def test_bn_eval_is_exact_and_nondegenerate(C, nhw, relu, residual):
    ref = A.bn_eval_reference(C, nhw, relu, residual)
    for mode in E.MODES:
        A.bn_eval_check_range(ref, mode)
    assert set(ref['var'].tolist()) <= {0.25, 1.0, 4.0} and set(ref['scale'].tolist()) <= {0.5, 1.0, 2.0}
    # (with a ReLU a channel whose beta - mean scale is low enough is closed everywhere: legitimate data)
    A.nondegenerate(ref['y'], 'y', 0.3 if relu else 0.5, 1 if relu else 3)
    A.nondegenerate(ref['dx'], 'dx', 0.25 if relu else 0.5, 1 if relu else 3)
    if relu:
        assert 0.2 <= float((ref['z'] > 0).double().mean()) <= 0.8


# ---------------------------------------------------------------------------------------------------------------------
# the other ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op,C,hw', [pytest.param(*c, id=A.pool_id(*c)) for c in A.POOL_CASES])
def test_pool_is_exact_and_nondegenerate(op, C, hw):
    ref = A.pool_reference(op, C, hw)
    shift = 2 if op[0] == 'avg' else 0
    _range_all_modes({k: ref[k] for k in ('x', 'gy', 'y', 'dx', 'add', 'dx_add')}, shift)
    A.nondegenerate(ref['y'], 'y')
    if op[0] == 'avg':
        A.nondegenerate(ref['dx'][:, :, :hw[0] // 2 * 2, :hw[1] // 2 * 2], 'dx')
        # the odd last row / column no window reaches has a zero gradient
        assert int(ref['dx'][:, :, hw[0] // 2 * 2:].count_nonzero()) == 0
        assert int(ref['dx'][:, :, :, hw[1] // 2 * 2:].count_nonzero()) == 0
    else:
        # tie-heavy: most windows hold their maximum more than once, and the gradient goes to one tap only
        k, s, p, ceil = op[1:]
        xp = F.pad(ref['x'], (p, k, p, k), value=-9.0)
        win = xp.unfold(2, k, s).unfold(3, k, s)[:, :, :ref['y'].shape[2], :ref['y'].shape[3]]
        ties = (win == ref['y'][..., None, None]).sum((-1, -2))
        assert int(ties.min()) >= 1 and float((ties > 1).double().mean()) >= 0.15
        assert float((ref['dx'] != 0).double().mean()) >= 0.1
    A.nondegenerate(ref['dx_add'], 'dx + add')


@pytest.mark.parametrize('C,H,W', A.GAP_CASES)
def test_gap_is_exact_and_nondegenerate(C, H, W):
    for c in sorted({A.chans(C, m) for m in E.MODES}):
        ref = A.gap_reference(c, H, W)
        shift = (H * W).bit_length() - 1
        assert 2 ** shift == H * W
        _range_all_modes({k: ref[k] for k in ('y', 'dx')}, shift)
        _range_all_modes({k: ref[k] for k in ('x', 'gy')})
        A.nondegenerate(ref['y'], 'y', 0.5, 1)   # (two values per channel: the variety is checked over all of y)
        A.nondegenerate(ref['dx'], 'dx', 1.0, 1)
        assert len(set(ref['y'].flatten().tolist())) >= 8


@pytest.mark.parametrize('act', A.ADD_ACTS, ids=str)
@pytest.mark.parametrize('n', A.ADD_N)
def test_add_is_exact_and_nondegenerate(n, act):
    ref = A.add_reference(n, act)
    _range_all_modes({'y': ref['y'], 'dx': ref['dx'], 'gy': ref['gy']}, E.act_shift(act))
    _range_all_modes({f'x{i}': t for i, t in enumerate(ref['xs'])})
    A.nondegenerate(ref['y'], 'y', 0.3 if act == 'relu' else 0.5)
    A.nondegenerate(ref['dx'], 'dx', 0.25 if act == 'relu' else 0.5)
    assert ref['y'].numel() % (256 * 8) != 0 and ref['y'].numel() % (256 * 4) != 0   # a partial last workgroup


@pytest.mark.parametrize('widths', A.CAT_WIDTHS, ids=str)
def test_cat_is_exact_and_nondegenerate(widths):
    ref = A.cat_reference(widths)
    _range_all_modes({'y': ref['y'], 'gy': ref['gy']})
    A.nondegenerate(ref['y'], 'y')
    for t in ref['dxs']:
        A.nondegenerate(t, 'dx')
    assert sum(widths) % 8 != 0 or any(w % 8 for w in widths)   # ragged: padding channels exist somewhere


@pytest.mark.parametrize('ca,cb,hwa,hwb', A.CROP_CASES)
def test_crop_is_exact_and_nondegenerate(ca, cb, hwa, hwb):
    ref = A.crop_reference(ca, cb, hwa, hwb)
    _range_all_modes({k: ref[k] for k in ('a', 'b', 'gy', 'y', 'da', 'db')})
    A.nondegenerate(ref['y'], 'y')
    for k, hw in (('da', hwa), ('db', hwb)):
        H, W = ref['y'].shape[2:]
        oy, ox = (hw[0] - H) // 2, (hw[1] - W) // 2
        inner = ref[k][:, :, oy:oy + H, ox:ox + W]
        A.nondegenerate(inner, k)
        assert int(ref[k].count_nonzero()) == int(inner.count_nonzero())   # zero outside the crop


@pytest.mark.parametrize('act', A.ACT_BWD, ids=str)
def test_act_bwd_hits_the_boundaries(act):
    ref = A.act_bwd_reference(act)
    _range_all_modes(ref, E.act_shift(act))
    y = ref['y']
    assert int((y == 0).sum()) >= 100 and int((y == 6).sum()) >= 100 and int((y < 0).sum()) >= 100
    # the reference is PyTorch's own derivative at those points
    z = y.clone().requires_grad_(True)
    E.apply_act(z, act).backward(ref['gy'])
    assert torch.equal(z.grad, ref['gx'])


@pytest.mark.parametrize('C,hw,size,ac', [pytest.param(*c, id=A.resize_id(*c)) for c in A.RESIZE_CASES])
def test_resize_is_exact_and_nondegenerate(C, hw, size, ac):
    ref = A.resize_reference(C, hw, size, ac)
    _range_all_modes({'y': ref['y'], 'dx': ref['dx']}, A.RESIZE_SHIFT)
    _range_all_modes({'x': ref['x'], 'gy': ref['gy']})
    A.nondegenerate(ref['y'], 'y')
    A.nondegenerate(ref['dx'], 'dx')
    # the weights really are dyadic: some output lies strictly between its taps
    assert not torch.equal(ref['y'], ref['y'].round()) or size[0] < hw[0]


def test_dropout_operands_are_nonzero_integers():
    x, gy = A.dropout_operands()
    assert bool((x != 0).all()) and bool((gy != 0).all()) and x.numel() % 4 == 0
    _range_all_modes({'4x': 4 * x, '4gy': 4 * gy})


def test_one_wrong_element_fails_the_bound(capsys):
    ref = A.avgpool3_random(16, (9, 7), 'bf16')
    good = ref['y'].to(torch.bfloat16)
    A.assert_bounded(good, ref['y'], ref['My'], A.AVG3_K_FWD, 'bf16', 'y')
    bad = good.clone()
    bad[1, 5, 2, 3] = (bad[1, 5, 2, 3].double() + A.ulp_store(ref['y'][1, 5, 2, 3], 'bf16')).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        A.assert_bounded(bad, ref['y'], ref['My'], A.AVG3_K_FWD, 'bf16', 'y')
    assert '1 of' in capsys.readouterr().out


@pytest.mark.parametrize('mode', E.MODES)
def test_ulp_store(mode):
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 3e-3, 100.0], dtype=torch.float64)
    dt = E.TORCH_DTYPE[mode]
    nxt = torch.nextafter(v.to(dt), torch.tensor(float('inf'), dtype=dt)).double()
    assert torch.equal(A.ulp_store(v.to(dt).double(), mode), nxt - v.to(dt).double())


# ---------------------------------------------------------------------------------------------------------------------
# Tier B: the references keep clear of the activation boundary
# ---------------------------------------------------------------------------------------------------------------------
def _bn_random_cases():
    return [pytest.param(C, nhw, mode, id=f'{A.bn_id(A.chans(C, mode), nhw)}-{mode}')
            for C, nhw in A.BN_CASES for mode in E.MODES]


@pytest.mark.parametrize('relu,residual', [f for f in A.BN_FLAGS if f[0]])
@pytest.mark.parametrize('C,nhw,mode', _bn_random_cases())
def test_bn_random_keeps_clear_of_zero(C, nhw, mode, relu, residual):
    ref = A.bn_train_random(A.chans(C, mode), nhw, relu, residual, mode)
    bound = 0.5 * A.ulp_store(ref['z'], mode) + A.BN_K_FWD * A.U24 * ref['My']
    assert bool((ref['z'].abs() > bound).all())
    assert torch.equal(A.q(ref['x'], mode), ref['x'])   # the redrawn inputs are still storage values
    assert 0.2 <= float((ref['z'] > 0).double().mean()) <= 0.8
    A.bn_train_random.cache_clear()


def test_resize_taps_are_the_taps_of_interpolate():
    """the unweighted tap matrices behind M select exactly the inputs F.interpolate reads"""
    for C, hw, size, ac in A.RESIZE_RANDOM:
        ref = A.resize_random(C, hw, size, ac, 'f32')
        x = torch.zeros(1, 1, *hw, dtype=torch.float64)
        for h in range(hw[0]):
            for w in range(hw[1]):
                x.zero_()
                x[0, 0, h, w] = 1.0
                y = F.interpolate(x, size=size, mode='bilinear', align_corners=ac)[0, 0]
                reach = torch.outer(ref['th'][:, h], ref['tw'][:, w]) > 0
                assert bool((reach | (y == 0)).all())
