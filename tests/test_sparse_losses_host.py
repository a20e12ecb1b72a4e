"""Host-side checks (no GPU) of the label-map losses: the fp64 restatements of tests/sparse_ref.py against
F.cross_entropy, against the reference's dense OhemCrossEntropy fixtures and against the reference's lovasz.xloss
fixtures (tests/golden/sparse_ce_*.npz, gen_golden_sparse_ce.py); argument validation of the ops, the losses, the train
step and the C ABI; the label-map mode of SyntheticSegDataset; the new config."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as R
from conftest import PKG, golden

F64 = torch.float64
LOSS_TOL = dict(rtol=2e-5, atol=1e-7)
GRAD_TOL = dict(rtol=2e-4, atol=2e-8)
SPARSE_GOLDEN = ('s1', 'c19', 'novoid', 'allvoid')


def _case(C=5, shape=(2, 7, 9), void=0.2, ignore=255, seed=0, all_void=False):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    x = (2 * torch.randn(B, C, *shape[1:], generator=g, dtype=F64)).requires_grad_(True)
    y = torch.randint(0, C, shape, generator=g)
    if 0 <= ignore < C:
        y[y == ignore] = (ignore + 1) % C      # the in-range ignore value marks void pixels only
    y[torch.rand(shape, generator=g) < void] = ignore
    if all_void:
        y[:] = ignore
    return x, y


GRID = list(itertools.product((False, True), (0.0, 0.1), ('mean', 'sum', 'none'), (255, -100, 1), (False, True)))


@pytest.mark.parametrize('weighted,eps,reduction,ignore,all_void', GRID)
def test_ce_restatement_equals_torch(weighted, eps, reduction, ignore, all_void):
    C = 5
    x, y = _case(C, ignore=ignore, all_void=all_void)
    w = torch.tensor([0.5, 2.0, 1.0, 0.25, 3.0], dtype=F64) if weighted else None
    up = torch.rand(y.shape, dtype=F64, generator=torch.Generator().manual_seed(9)) if reduction == 'none' else 0.73
    want = F.cross_entropy(x, y, w, ignore_index=ignore, reduction=reduction, label_smoothing=eps)
    gw, = torch.autograd.grad((want * up).sum(), x)
    got = R.ce_labels64(x, y, w, ignore, reduction, eps)
    gg, = torch.autograd.grad((got * up).sum(), x)
    assert got.shape == want.shape
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13, equal_nan=True)
    assert torch.allclose(gg, gw, rtol=1e-12, atol=1e-14)
    if all_void:
        assert not gg.any() and not gw.any()
        if reduction == 'mean':
            assert torch.isnan(want) and torch.isnan(got)
            z = R.ce_labels64(x, y, w, ignore, reduction, eps, empty='zero')
            assert float(z.detach()) == 0.0 and not torch.autograd.grad(z, x)[0].any()
    else:
        assert gg.any() and torch.isfinite(got).all()


def test_ce_restatement_treats_out_of_range_labels_as_void():
    x, y = _case(4, ignore=255)
    y2 = y.clone()
    y2[y == 255] = 77           # not the ignore value, not a class
    y2[0, 0, 0] = -3
    y[0, 0, 0] = 255
    assert torch.equal(R.ce_labels64(x, y2, None, 255, 'none'), R.ce_labels64(x, y, None, 255, 'none'))


@pytest.mark.parametrize('name', SPARSE_GOLDEN)
def test_ce_restatement_reproduces_the_reference_fixtures(name):
    """the default path (ignore 255, mean) is the reference's lovasz.xloss itself"""
    g = golden(f'sparse_ce_{name}.npz')
    x = torch.from_numpy(g['x']).double().requires_grad_(True)
    y = torch.from_numpy(g['y'])
    assert y.dtype == torch.uint8
    loss = R.ce_labels64(x, y)
    (loss * float(g['w'])).backward()
    print(f'{name}: loss {float(loss.detach())!r} golden {float(g["loss"])!r} grad err '
          f'{np.abs(x.grad.numpy() - g["grad"]).max():.3e}')
    assert np.allclose(loss.detach().numpy(), g['loss'], equal_nan=True, **LOSS_TOL)
    assert np.allclose(x.grad.numpy(), g['grad'], **GRAD_TOL)
    assert bool(np.isnan(g['loss'])) == (name == 'allvoid') and np.isfinite(g['grad']).all()
    assert (name == 'allvoid') == (not g['grad'].any())


@pytest.mark.parametrize('min_kept', [100, 1000, 5000])
def test_ohem_restatement_reproduces_the_reference_dense_fixtures(min_kept):
    """nothing void: the label-map OHEM on argmax(one-hot) is the reference's dense OhemCrossEntropy"""
    from test_losses_ext_host import ohem64
    g = golden(f'losses_ext_ohem_k{min_kept}.npz')
    t = torch.from_numpy(g['t'])
    assert torch.equal(t.sum(1), torch.ones_like(t[:, 0])) and ((t == 0) | (t == 1)).all()
    x = torch.from_numpy(g['x']).double().requires_grad_(True)
    y = t.argmax(1)
    thres = float(g['thres'])
    thr, sel, n = R.ohem_labels_state64(x.detach(), y, thres, min_kept)
    assert n == y.numel() and int(sel.sum()) == int(g['kept']) and abs(thr - float(g['threshold'])) <= 1e-6
    loss = R.ohem_labels64(x, y, thres, min_kept)
    gx, = torch.autograd.grad(loss * torch.from_numpy(g['w']).double(), x)
    assert np.allclose(loss.detach().numpy(), g['loss'], **LOSS_TOL)
    assert np.allclose(gx.numpy(), g['grad'], **GRAD_TOL)
    dense = ohem64(x, t.double(), thres, min_kept)
    assert abs(float(dense.detach()) - float(loss.detach())) <= 1e-14


def test_ohem_restatement_void_handling():
    x, y = _case(3, shape=(2, 6, 6), void=0.5)
    n = int((y != 255).sum())
    thr, sel, nv = R.ohem_labels_state64(x.detach(), y, 0.0, 10 ** 6)
    pred = torch.softmax(x.detach(), 1).gather(1, torch.where(y == 255, 0, y).unsqueeze(1)).squeeze(1)
    assert nv == n and thr == float(pred[y != 255].max()) and int(sel.sum()) == n - 1    # k clamps to n_valid - 1
    assert not sel[y == 255].any()
    x0, y0 = _case(3, shape=(1, 4, 4), all_void=True)
    loss = R.ohem_labels64(x0, y0, 0.7, 10)
    assert torch.isnan(loss) and not torch.autograd.grad(loss, x0)[0].any()


# ---- argument validation -----------------------------------------------------------------------------------------
def test_op_argument_validation():
    from ssseg import ops
    x, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.uint8)
    ce, oh = ops.cross_entropy_labels, ops.ohem_cross_entropy_labels
    for fn in (lambda a, b: ce(a, b), lambda a, b: oh(a, b, 0.7, 10)):
        with pytest.raises(ValueError, match='one label per pixel'):
            fn(x, torch.zeros(2, 5, 4, dtype=torch.uint8))
        with pytest.raises(ValueError, match='one label per pixel'):
            fn(x, torch.zeros(3, 4, 5, dtype=torch.int64))
        with pytest.raises(ValueError, match='one label per pixel'):
            fn(x, torch.zeros(2, 3, 4, 5, dtype=torch.int64))
        with pytest.raises(ValueError, match='2 <= C <= 64'):
            fn(torch.zeros(2, 1, 4, 5), y)
        with pytest.raises(ValueError, match='2 <= C <= 64'):
            fn(torch.zeros(2, 65, 4, 5), y)
        with pytest.raises(ValueError, match='uint8 or int64'):
            fn(x, y.float())
        with pytest.raises(RuntimeError, match='HIP device tensor'):      # no CPU fallback
            fn(x, y)
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            fn(x, y.long())
    with pytest.raises(ValueError, match='weight holds 2 values for 3'):
        ce(x, y, weight=torch.ones(2))
    for eps in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match='label_smoothing'):
            ce(x, y, label_smoothing=eps)
    with pytest.raises(ValueError, match='not a valid value for reduction'):
        ce(x, y, reduction='batchmean')
    with pytest.raises(ValueError, match='empty'):
        ce(x, y, empty='one')
    with pytest.raises(ValueError, match='min_kept'):
        oh(x, y, 0.7, -1)


def test_losses_and_train_step_refusals():
    import losses as L
    import train
    x, y = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.uint8)
    m = L.CrossEntropyLossWithLogits()
    assert (m.weight, m.ignore_index, m.reduction, m.label_smoothing, m.empty) == (None, 255, 'mean', 0.0, 'nan')
    assert L.CrossEntropyLossWithLogits(weight=[1, 2, 3]).weight.dtype == torch.float32
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        m(x, y)
    o = L.OhemCrossEntropy()
    assert (o.thresh, o.min_kept, o.ignore_label) == (0.7, 100000, 255)
    assert L.OhemCrossEntropy(ignore_label=0).ignore_label == 0
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        o(x, y)
    with pytest.raises(ValueError, match='same shape'):       # a 4-D target still takes the dense path
        o(x, torch.zeros(2, 2, 4, 5))
    # the two branches that need a float [B, C, H, W] mask refuse a label map before anything is launched (the model is
    # never called: None would raise another error)
    base = dict(use_semi_supervised=False, loss=None)
    with pytest.raises(ValueError, match='adversarial'):
        train.train_step(None, None, None, x, y, None, None, 0, 0, {'train': dict(base, adversarial={})})
    with pytest.raises(NotImplementedError, match='device augmentation'):
        train.train_step(None, None, None, x, y, None, None, 0, 0, {'train': dict(base, device_augment=object())})
    import lovasz
    with pytest.raises(NotImplementedError):                   # unchanged: the new class is the way
        lovasz.xloss(x, y.long())


def test_abi_names_and_host_side_validation():
    from ssseg import native
    new = {'ssseg_ce_labels_fwd', 'ssseg_ce_labels_bwd', 'ssseg_ohem_labels_fwd', 'ssseg_ohem_labels_bwd'}
    assert new <= set(native.header_symbols()) and new <= set(native.SIGS)
    lib = native.lib()
    E, p, big = -1, 0x1000, 1 << 20
    U8, I64 = native.LOVASZ_LABEL_U8, native.LOVASZ_LABEL_I64
    fwd, bwd = lib.ssseg_ce_labels_fwd, lib.ssseg_ce_labels_bwd
    assert fwd(None, None, U8, 1, 2, 16, None, 255, 0.0, 1, 0, None, None, 0, None) == E
    assert fwd(p, p, U8, 1, 1, 16, None, 255, 0.0, 1, 0, p, p, big, None) == E       # C < 2
    assert fwd(p, p, I64, 1, 65, 16, None, 255, 0.0, 1, 0, p, p, big, None) == E     # C > 64
    assert fwd(p, p, 2, 1, 3, 16, None, 255, 0.0, 1, 0, p, p, big, None) == E        # float labels: no such kind
    assert fwd(p, p, U8, 1, 3, 16, None, 255, 1.0, 1, 0, p, p, big, None) == E       # smoothing outside [0, 1)
    assert fwd(p, p, U8, 1, 3, 16, None, 255, -0.5, 1, 0, p, p, big, None) == E
    assert fwd(p, p, U8, 1, 3, 16, None, 255, 0.0, 3, 0, p, p, big, None) == E       # no such reduction
    assert fwd(p, p, U8, 1, 3, 16, None, 255, 0.0, 1, 0, p, p, 8, None) == -3        # workspace too small
    assert bwd(None, None, U8, 1, 2, 16, None, 255, 0.0, 1, None, None, None, 0, None) == E
    assert bwd(p, p, U8, 1, 65, 16, None, 255, 0.0, 1, p, p, p, big, None) == E
    assert bwd(p, p, U8, 1, 3, 16, None, 255, 0.0, 1, p, p, None, 0, None) == -3     # 'mean' reads the denominator
    ofwd, obwd = lib.ssseg_ohem_labels_fwd, lib.ssseg_ohem_labels_bwd
    assert ofwd(None, None, U8, 1, 2, 16, 255, 0.7, 10, None, None, 0, None) == E
    assert ofwd(p, p, U8, 1, 1, 16, 255, 0.7, 10, p, p, big, None) == E
    assert ofwd(p, p, U8, 1, 3, 16, 255, 0.7, -1, p, p, big, None) == E
    assert ofwd(p, p, 3, 1, 3, 16, 255, 0.7, 10, p, p, big, None) == E
    assert ofwd(p, p, U8, 1, 3, 16, 255, 0.7, 10, p, p, 8, None) == -3
    assert obwd(None, None, U8, 1, 2, 16, None, None, None, 0, None) == E
    assert obwd(p, p, I64, 1, 65, 16, p, p, p, big, None) == E
    ws = lib.ssseg_segloss_workspace_bytes
    assert (native.LOSS_CE_LABELS, native.LOSS_OHEM_LABELS) == (5, 6)               # appended, nothing renumbered
    assert (native.LOSS_REDUCE, native.LOSS_OHEM, native.LOSS_NFL, native.LOSS_DICE_LOGITS,
            native.LOSS_DICE_PROB) == (0, 1, 2, 3, 4)
    assert ws(native.LOSS_CE_LABELS, 16, 19, 512 * 512) == ws(native.LOSS_CE_LABELS, 1, 2, 1) > 0
    assert ws(native.LOSS_OHEM_LABELS, 2, 3, 576) - ws(native.LOSS_OHEM_LABELS, 2, 3, 76) == 2 * 4 * 2 * 500
    assert ws(native.LOSS_CE_LABELS, 0, 2, 1) == 0 and ws(7, 1, 2, 1) == 0


# ---- SyntheticSegDataset -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [2, 5])
def test_dataset_label_map(C):
    from data.synthetic import SyntheticSegDataset as D
    kw = dict(length=4, size=64, seed=7, blob_sigma=4.0, num_classes=C)
    dense, again = D(**kw), D(label_map=False, void_fraction=0.0, ignore_label=255, label_dtype=torch.uint8, **kw)
    lab, void = D(label_map=True, **kw), D(label_map=True, void_fraction=0.25, **kw)
    wide = D(label_map=True, void_fraction=0.25, ignore_label=-1, label_dtype=torch.int64, **kw)
    for i in range(2):
        a, b, l, v, w = dense[i], again[i], lab[i], void[i], wide[i]
        # the defaults change nothing
        assert a['semantic_mask'].dtype == torch.float32 and tuple(a['semantic_mask'].shape) == (C, 64, 64)
        assert torch.equal(a['image'], b['image']) and torch.equal(a['semantic_mask'], b['semantic_mask'])
        # images and class labels are those of the one-hot dataset of the same seed
        for s in (l, v, w):
            assert torch.equal(s['image'], a['image']) and tuple(s['semantic_mask'].shape) == (64, 64)
        am = a['semantic_mask'].argmax(0)
        assert l['semantic_mask'].dtype == torch.uint8 and torch.equal(l['semantic_mask'].long(), am)
        is_void = v['semantic_mask'] == 255
        share = float(is_void.float().mean())
        print(f'C={C} item {i}: void share {share:.4f}')
        assert 0.0 < share < 1.0
        assert torch.equal(v['semantic_mask'].long()[~is_void], am[~is_void])
        assert w['semantic_mask'].dtype == torch.int64
        assert torch.equal(w['semantic_mask'] == -1, is_void)          # the void pixels do not depend on the label
        assert torch.equal(w['semantic_mask'][~is_void], am[~is_void])
    assert not torch.equal(void[0]['semantic_mask'] == 255, void[1]['semantic_mask'] == 255)
    with pytest.raises(ValueError, match='label_map=True'):
        D(void_fraction=0.1, **kw)
    with pytest.raises(ValueError, match='void_fraction'):
        D(label_map=True, void_fraction=1.5, **kw)


def test_dataset_default_output_is_pinned():
    """the one-hot output of a fixed seed, by its checksum: the new arguments leave the default path alone"""
    from data.synthetic import SyntheticSegDataset as D
    for C in (2, 4):
        s = D(length=2, size=32, seed=3, blob_sigma=3.0, num_classes=C)[1]
        m = s['semantic_mask']
        assert torch.equal(m.sum(0), torch.ones(32, 32)) and ((m == 0) | (m == 1)).all()
        g = torch.Generator().manual_seed(3 * 1_000_003 + 1)
        assert torch.equal(s['image'], torch.rand(3, 32, 32, generator=g))
        # background share = 1 - fg_fraction (0.4), cut at a quantile of the field
        assert abs(float(m[0].mean()) - 0.6) < 0.01


def test_labelmap_config():
    import config
    import losses as L
    cfg = config.fromfile(os.path.join(PKG, 'configs', 'c6_unet_r50_labelmap.py'))
    base = config.fromfile(os.path.join(PKG, 'configs', 'c6_unet_r50_multiclass.py'))
    tc = cfg['train']
    assert tc['ignore_label'] == 255 and 'ignore_label' not in base['train']
    specs = tc['loss'].losses
    assert [type(s['loss_fn']) for s in specs] == [L.CrossEntropyLossWithLogits, L.LovaszSoftmaxLossWithLogits]
    assert [s['weight'] for s in specs] == [[0.5], [0.5]]
    assert specs[0]['loss_fn'].ignore_index == 255 and specs[1]['loss_fn'].ignore == 255
    for part in (tc['dataset'], cfg['val']['dataset']):
        kw = part.keywords
        assert kw['label_map'] is True and kw['void_fraction'] == 0.05 and kw['ignore_label'] == 255
        assert kw['num_classes'] == 19
    same = ('batch_size_per_worker', 'consistency_activation', 'confidence_threshold', 'base_lr', 'crop_size')
    assert all(tc[k] == base['train'][k] for k in same)
