"""CPU: the fp64 restatement of the pseudo-label consistency loss (tests/pseudo_ce_ref.py) against a direct per-pixel
loop, the new C ABI symbols' host-side refusals, and the configuration keys of the training step."""
import numpy as np
import pytest
import torch

import multiclass_ref as R
import pseudo_ce_ref as P

THR = 0.7


@pytest.mark.parametrize('weighting', ['pixel', 'batch'])
def test_restatement_equals_the_pixel_loop(weighting):
    shape = (2, 3, 7, 9)
    g = torch.Generator().manual_seed(5)
    s = torch.randn(*shape, generator=g, dtype=torch.float64)
    t, conf = R.confident_teacher(shape, THR, seed=5)
    t = t.double()
    assert 0 < int(conf.sum()) < conf.numel()
    w = torch.rand(2, 7, 9, generator=g, dtype=torch.float64)
    w[0, 0, :4] = 0.0
    for weight in (None, w):
        loss, cm_mean, s_cm, n_w = P.pseudo_ce(s, t, THR, weight, weighting)
        want = P.pseudo_ce_loop(s, t, THR, weight, weighting)
        print(weighting, 'w' if weight is not None else 'no w', float(loss), want)
        assert np.allclose(float(loss), want[0], rtol=1e-13, atol=0)
        assert np.allclose(float(cm_mean), want[1], rtol=1e-13, atol=0)
        assert np.allclose(float(s_cm), want[2], rtol=1e-13, atol=0) and np.allclose(float(n_w), want[3], rtol=1e-13)
        if weight is None:
            assert float(s_cm) == float(conf.sum()) and float(n_w) == conf.numel()
        # the analytic gradient of the header: k (softmax(s)_c - [c == y])
        _, _, _, grad = P.pseudo_ce_grad(s, t, THR, weight, weighting, gout=0.7)
        wt = torch.ones(2, 7, 9, dtype=torch.float64) if weight is None else weight
        k = wt * conf.double() / n_w if weighting == 'pixel' else (s_cm / n_w) * wt / n_w
        onehot = torch.nn.functional.one_hot(t.argmax(1), 3).permute(0, 3, 1, 2).double()
        want_g = 0.7 * k.unsqueeze(1) * (torch.softmax(s, 1) - onehot)
        assert np.allclose(grad, want_g.numpy(), rtol=1e-11, atol=1e-16)
        if weighting == 'pixel':
            assert np.all(grad.transpose(0, 2, 3, 1)[~conf.numpy()] == 0)
    # the two weightings are two losses (what the mutated-copy test of test_pseudo_ce.py relies on)
    assert not np.allclose(float(P.pseudo_ce(s, t, THR, None, 'pixel')[0]), float(P.pseudo_ce(s, t, THR, None, 'batch')[0]),
                           rtol=1e-3)


def test_restatement_no_confident_pixel_is_zero():
    s = torch.randn(2, 3, 7, 9, dtype=torch.float64)
    t, _ = R.confident_teacher((2, 3, 7, 9), THR, seed=1)
    loss, cm, s_cm, n_w = P.pseudo_ce(s, t.double(), 1.0)
    assert float(loss) == 0.0 and float(cm) == 0.0 and float(n_w) == 2 * 7 * 9
    s[0, 1, 2, 3] = float('nan')
    assert float(P.pseudo_ce(s, t.double(), 1.0)[0]) == 0.0         # selected, not multiplied
    assert np.isnan(float(P.pseudo_ce(s, t.double(), 1.0, weighting='batch')[0]))


def test_header_declares_the_entry_points_and_they_refuse_on_the_host():
    from ssseg import native
    new = {'ssseg_consistency_ce_fwd', 'ssseg_consistency_ce_bwd', 'ssseg_consistency_ce_workspace_bytes'}
    assert new <= set(native.header_symbols()) and new <= set(native.SIGS)
    lib = native.lib()
    nb = lib.ssseg_consistency_ce_workspace_bytes(1 << 20)
    assert nb == 8 * 3 * 1024 and nb > lib.ssseg_reduce_workspace_bytes(1 << 20)
    # null pointers -> SSSEG_EINVAL
    assert lib.ssseg_consistency_ce_fwd(None, None, None, 1, 3, 8, 0.5, 0, None, None, 0, None) == -1
    assert lib.ssseg_consistency_ce_bwd(None, None, None, 1, 3, 8, 0.5, 0, None, None, None, None) == -1
    p = torch.zeros(1).data_ptr()     # never dereferenced: the arguments are refused first
    assert lib.ssseg_consistency_ce_fwd(p, p, None, 1, 65, 8, 0.5, 0, p, p, nb, None) == -1
    assert lib.ssseg_consistency_ce_fwd(p, p, None, 1, 0, 8, 0.5, 0, p, p, nb, None) == -1
    assert lib.ssseg_consistency_ce_bwd(p, p, None, 1, 65, 8, 0.5, 0, p, p, p, None) == -1
    for bad in (2, -1):
        assert lib.ssseg_consistency_ce_fwd(p, p, None, 1, 3, 8, 0.5, bad, p, p, nb, None) == -1
        assert lib.ssseg_consistency_ce_bwd(p, p, None, 1, 3, 8, 0.5, bad, p, p, p, None) == -1
    # the two-slot reduction workspace is too small -> SSSEG_EWORKSPACE
    assert lib.ssseg_consistency_ce_fwd(p, p, None, 1, 3, 8, 0.5, 0, p, p, lib.ssseg_reduce_workspace_bytes(8),
                                        None) == -3


def test_op_refuses_bad_arguments_on_the_host():
    from ssseg import ops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match='weighting'):
        ops.consistency_loss_ce(x, x, THR, weighting='mean')
    with pytest.raises(ValueError, match='one shape'):
        ops.consistency_loss_ce(x, x[:, :2], THR)
    with pytest.raises(ValueError, match='65 channels'):
        ops.consistency_loss_ce(torch.zeros(1, 65, 2, 2), torch.zeros(1, 65, 2, 2), THR)
    with pytest.raises(ValueError, match='one weight per pixel'):
        ops.consistency_loss_ce(x, x, THR, w=torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.consistency_loss_ce(x, x, THR)


def test_config_validation():
    import train
    base = {'consistency_activation': 'softmax'}
    assert train._consistency_loss_kind({}) == ('mse', None)
    assert train._consistency_loss_kind({'consistency_loss': 'mse'}) == ('mse', None)
    assert train._consistency_loss_kind(dict(base, consistency_loss='mse')) == ('mse', None)
    assert train._consistency_loss_kind(dict(base, consistency_loss='ce')) == ('ce', 'pixel')
    assert train._consistency_loss_kind(dict(base, consistency_loss='ce', consistency_ce_weighting='batch')) == \
        ('ce', 'batch')
    with pytest.raises(ValueError, match='consistency_loss'):
        train._consistency_loss_kind(dict(base, consistency_loss='kl'))
    with pytest.raises(ValueError, match='consistency_ce_weighting'):
        train._consistency_loss_kind(dict(base, consistency_loss='ce', consistency_ce_weighting='image'))
    with pytest.raises(ValueError, match='softmax'):
        train._consistency_loss_kind({'consistency_loss': 'ce'})
    with pytest.raises(ValueError, match='softmax'):
        train._consistency_loss_kind({'consistency_loss': 'ce', 'consistency_activation': 'sigmoid'})


def test_train_step_refuses_before_anything_is_launched():
    """the refusal comes before the model's first forward: the model here would raise another error if it were called"""
    import train

    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError('the model was called')
    x = torch.zeros(2, 3, 8, 8)
    for bad in ({'consistency_loss': 'kl'}, {'consistency_loss': 'ce'},
                {'consistency_loss': 'ce', 'consistency_activation': 'softmax', 'consistency_ce_weighting': 'x'}):
        tc = dict(use_semi_supervised=True, virtual_batch_size_multiplier=1, **bad)
        with pytest.raises(ValueError, match='consistency'):
            train.train_step(Never(), Never(), None, x, x, x, x, 26, 0, {'train': tc})


def test_new_configs_load_and_select_the_loss():
    import os
    import config
    import mixmasks
    import train
    here = os.path.join(os.path.dirname(os.path.abspath(config.__file__)), 'configs')
    want = {'c6_unet_r50_classmix_ce.py': ('classmix', ('ce', 'batch')),
            'c6_unet_r50_cutmix_ce.py': ('cutmix', ('ce', 'pixel')),
            'c6_unet_r50_classmix.py': ('classmix', ('mse', None))}
    for name, (mask, kind) in want.items():
        cfg = config.fromfile(os.path.join(here, name))
        tc = cfg['train']
        assert mixmasks.mix_mask_kind(tc) == mask and train._consistency_loss_kind(tc) == kind, name
