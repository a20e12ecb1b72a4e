"""CPU: the fp64 restatement of the self-adaptive confidence thresholds (tests/adaptive_thr_ref.py) against a direct
per-pixel loop, the designed teacher of the GPU tests, the new C ABI symbols' host-side refusals, the configuration keys
of the training step and the host side of ops.AdaptiveThreshold."""
import numpy as np
import pytest
import torch

import adaptive_thr_ref as A
import pseudo_ce_ref as P


@pytest.mark.parametrize('momentum', [0.0, 0.5, 0.999])
def test_restatement_equals_the_pixel_loop(momentum):
    shape = (2, 3, 5, 7)
    state = A.sat_init(3)
    tau, ptilde = 1.0 / 3, [1.0 / 3] * 3
    for k in range(3):
        t = torch.randn(*shape, generator=torch.Generator().manual_seed(20 + k)) * 4
        thr, m, q = A.sat_update(state, t, momentum)
        tau, ptilde, want_thr = A.sat_update_loop(tau, ptilde, t, momentum)
        print(momentum, k, float(state['tau']), tau, thr.tolist(), want_thr)
        assert np.allclose(float(state['tau']), tau, rtol=1e-13, atol=0)
        assert np.allclose(state['ptilde'].numpy(), ptilde, rtol=1e-13, atol=0)
        assert np.allclose(thr.double().numpy(), want_thr, rtol=2e-7, atol=0) and thr.dtype == torch.float32
        assert abs(float(q.sum()) - 1.0) < 1e-12 and 1.0 / 3 <= float(m) <= 1.0
    assert state['steps'] == 3
    if momentum == 0.0:      # the state is the last batch's statistics
        assert float(state['tau']) == float(m) and torch.equal(state['ptilde'], q)
    # the class with the largest ptilde has thr == tau; every other class a lower one
    top = int(state['ptilde'].argmax())
    assert float(thr[top]) == float(state['tau'].float()) and all(float(thr[c]) < float(thr[top]) for c in range(3)
                                                                   if c != top)


def test_restatement_ce_with_a_threshold_vector_equals_the_pixel_loop():
    shape = (2, 3, 7, 9)
    t = A.tiered_teacher(shape, 5)
    thr_c = torch.tensor([0.6, 0.9, 0.6])
    assert A.min_distance(t, thr_c) >= 1e-3
    g = torch.Generator().manual_seed(5)
    s = torch.randn(*shape, generator=g, dtype=torch.float64)
    w = torch.rand(2, 7, 9, generator=g, dtype=torch.float64)
    y = torch.argmax(t, 1)
    for weighting in ('pixel', 'batch'):
        for weight in (None, w):
            loss, cm_mean, s_cm, n_w = A.pseudo_ce(s, t.double(), thr_c, weight, weighting)
            # class by class: the scalar loop with that class's threshold on that class's pixels
            n = sc = sconf = sall = 0.0
            for c in range(3):
                wc = (y == c).double() * (1.0 if weight is None else weight)
                lc, _, scc, nc = P.pseudo_ce_loop(s, t.double(), float(thr_c[c]), wc, 'pixel')
                la, _, _, _ = P.pseudo_ce_loop(s, t.double(), -1.0, wc, 'pixel')   # every pixel confident: sum w ce
                n, sc, sconf, sall = n + nc, sc + scc, sconf + lc * nc, sall + la * nc
            want = sconf / n if weighting == 'pixel' else (sc / n) * (sall / n)
            print(weighting, float(loss), want, float(s_cm), sc)
            assert np.allclose(float(loss), want, rtol=1e-12, atol=0)
            assert np.allclose(float(s_cm), sc, rtol=1e-13, atol=0) and np.allclose(float(n_w), n, rtol=1e-13)
    # the 0.75 tier is confident in the even classes only, the 0.99 tier everywhere, the tie tier nowhere
    conf, _ = A.confidence(t)
    on = A.confident(t, thr_c)
    mid = (conf - 0.75).abs() < 1e-3
    assert torch.equal(on[mid], (y[mid] % 2 == 0)) and on[(conf - 0.99).abs() < 1e-3].all()
    assert not on[(conf - 0.5).abs() < 1e-3].any() and 0 < int(mid.sum()) and 0 < int(on.sum()) < on.numel()


@pytest.mark.parametrize('C', [2, 3, 5, 19])
def test_tiered_teacher_is_what_it_says(C):
    shape = (2, C, 17, 31)
    t = A.tiered_teacher(shape, A.TIER_SEED)
    assert t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
    conf, y = A.confidence(t)
    tiers = [((conf - v).abs() < 1e-4) for v in (0.99, 0.75, 0.5)]
    frac = [float(m.float().mean()) for m in tiers]
    print(C, frac, torch.bincount(y.flatten(), minlength=C).tolist())
    assert sum(int(m.sum()) for m in tiers) == conf.numel()
    assert all(abs(f - want) < 0.06 for f, want in zip(frac, A.TIERS))
    # the tie is exact: two equal maxima, and torch.argmax takes the first
    top2 = t.double().topk(2, dim=1).values
    assert torch.equal(top2[:, 0][tiers[2]], top2[:, 1][tiers[2]]) and (top2[:, 0] > top2[:, 1])[~tiers[2]].all()
    # three updates with momentum 0 and 0.5: no pixel within 1e-3 of its own threshold, both kinds of pixel present, and
    # the per-class thresholds decide otherwise than the scalar tau would
    for momentum in (0.0, 0.5):
        state = A.sat_init(C)
        for k in range(3):
            tk = A.tiered_teacher(shape, A.TIER_SEED + k)
            thr, _, _ = A.sat_update(state, tk, momentum)
            dist, on = A.min_distance(tk, thr), A.confident(tk, thr)
            scalar = A.confidence(tk)[0] > float(state['tau'])
            print(C, momentum, k, 'distance', dist, 'confident', float(on.float().mean()), 'differs from the scalar in',
                  int((on != scalar).sum()))
            assert dist >= 1e-3
            if momentum == 0.0:
                assert 0 < int(on.sum()) < on.numel() and int((on != scalar).sum()) > 0
    # momentum 0.999: three steps move tau and every ptilde_c by less than 3 (1 - momentum) = 3e-3 (every statistic is
    # inside [0, 1]), thr stays near 1 / C and, from three classes on, every pixel is confident: this case checks the
    # EMA arithmetic only
    state = A.sat_init(C)
    for k in range(3):
        tk = A.tiered_teacher(shape, A.TIER_SEED + k)
        thr, _, _ = A.sat_update(state, tk, 0.999)
    print(C, 0.999, 'thr - 1/C', float((thr - 1.0 / C).abs().max()))
    assert 0 < abs(float(state['tau']) - 1.0 / C) <= 3e-3 and float((state['ptilde'] - 1.0 / C).abs().max()) <= 3e-3
    assert C == 2 or A.confident(tk, thr).all()


def test_header_declares_the_entry_points_and_they_refuse_on_the_host():
    from ssseg import native
    new = {'ssseg_adaptive_thr_update', 'ssseg_adaptive_thr_workspace_bytes', 'ssseg_consistency_ce_cls_fwd',
           'ssseg_consistency_ce_cls_bwd'}
    assert new <= set(native.header_symbols()) and new <= set(native.SIGS)
    lib = native.lib()
    assert [lib.ssseg_adaptive_thr_workspace_bytes(C) for C in (1, 19, 64)] == [8 * 1024 * (C + 1) for C in (1, 19, 64)]
    assert lib.ssseg_adaptive_thr_workspace_bytes(0) == 0 and lib.ssseg_adaptive_thr_workspace_bytes(65) == 0
    p = torch.zeros(1).data_ptr()     # never dereferenced: the arguments are refused first
    nb = lib.ssseg_adaptive_thr_workspace_bytes(3)
    upd = lib.ssseg_adaptive_thr_update
    # null pointers -> SSSEG_EINVAL
    assert upd(None, 1, 3, 8, 0.5, p, p, p, nb, None) == -1
    assert upd(p, 1, 3, 8, 0.5, None, p, p, nb, None) == -1
    assert upd(p, 1, 3, 8, 0.5, p, None, p, nb, None) == -1
    for B, C, HW in ((0, 3, 8), (-1, 3, 8), (1, 0, 8), (1, 65, 8), (1, -3, 8), (1, 3, 0), (1, 3, -8)):
        assert upd(p, B, C, HW, 0.5, p, p, p, 8 * 1024 * 66, None) == -1, (B, C, HW)
    for bad in (1.0, -0.1, 1.5, float('nan'), float('inf')):
        assert upd(p, 1, 3, 8, bad, p, p, p, nb, None) == -1, bad
    # a short or missing workspace -> SSSEG_EWORKSPACE (the three-slot workspace of the loss is too small for C = 3)
    assert upd(p, 1, 3, 8, 0.5, p, p, p, nb - 1, None) == -3
    assert upd(p, 1, 3, 8, 0.5, p, p, None, nb, None) == -3
    assert upd(p, 1, 3, 8, 0.5, p, p, p, lib.ssseg_consistency_ce_workspace_bytes(8), None) == -3
    # the _cls passes: a null threshold vector, and the scalar passes' refusals
    cnb = lib.ssseg_consistency_ce_workspace_bytes(8)
    fwd, bwd = lib.ssseg_consistency_ce_cls_fwd, lib.ssseg_consistency_ce_cls_bwd
    assert fwd(p, p, None, 1, 3, 8, None, 0, p, p, cnb, None) == -1
    assert bwd(p, p, None, 1, 3, 8, None, 0, p, p, p, None) == -1
    assert fwd(None, None, None, 1, 3, 8, p, 0, None, None, 0, None) == -1
    assert bwd(None, None, None, 1, 3, 8, p, 0, None, None, None, None) == -1
    assert fwd(p, p, None, 1, 65, 8, p, 0, p, p, cnb, None) == -1 and fwd(p, p, None, 1, 0, 8, p, 0, p, p, cnb, None) == -1
    assert bwd(p, p, None, 1, 65, 8, p, 0, p, p, p, None) == -1
    for bad in (2, -1):
        assert fwd(p, p, None, 1, 3, 8, p, bad, p, p, cnb, None) == -1
        assert bwd(p, p, None, 1, 3, 8, p, bad, p, p, p, None) == -1
    assert fwd(p, p, None, 1, 3, 8, p, 0, p, p, lib.ssseg_reduce_workspace_bytes(8), None) == -3


def test_op_refuses_a_bad_threshold_vector_on_the_host():
    from ssseg import ops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match='one per class'):
        ops.consistency_loss_ce(x, x, torch.zeros(4))
    with pytest.raises(ValueError, match='one per class'):
        ops.consistency_loss_ce(x, x, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match='one per class'):
        ops.consistency_loss_ce(x, x, torch.zeros(1, 3))
    with pytest.raises(ValueError, match='HIP device tensor'):      # the logits' own check comes first
        ops.consistency_loss_ce(x, x, torch.zeros(3))
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.AdaptiveThreshold().update(x)
    with pytest.raises(ValueError, match='1 <= C <= 64'):
        ops.AdaptiveThreshold().update(torch.zeros(1, 65, 2, 2))
    for bad in (1.0, -0.5, float('nan')):
        with pytest.raises(ValueError, match='momentum'):
            ops.AdaptiveThreshold(bad)
    with pytest.raises(ValueError, match='classes'):
        ops.AdaptiveThreshold(num_classes=65)


def test_state_dict_round_trip_on_the_host():
    from ssseg import ops
    a = ops.AdaptiveThreshold(0.5)
    assert a.state_dict() == {} and a.num_classes is None and a.tau() is None
    a = ops.AdaptiveThreshold(0.5, num_classes=4)
    assert a.state_dict() == {'tau': 0.25, 'ptilde': [0.25] * 4, 'steps': 0} and a.tau() == 0.25
    sd = {'tau': 0.8125, 'ptilde': [0.5, 0.25, 0.125, 0.125], 'steps': 7}
    a.load_state_dict(sd)
    assert a.state_dict() == sd and a.state_dict() is not sd and a.num_classes == 4
    b = ops.AdaptiveThreshold()                 # the class count comes with the state
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == sd and b.num_classes == 4
    # through torch.save / torch.load(weights_only=True), as the trainer's checkpoint does
    import io
    buf = io.BytesIO()
    torch.save({'confidence_threshold_state': b.state_dict()}, buf)
    buf.seek(0)
    c = ops.AdaptiveThreshold(num_classes=4)
    c.load_state_dict(torch.load(buf, weights_only=True)['confidence_threshold_state'])
    assert c.state_dict() == sd
    with pytest.raises(ValueError, match='3 classes'):
        c.load_state_dict({'tau': 0.5, 'ptilde': [0.5, 0.25, 0.25], 'steps': 1})
    assert c.state_dict() == sd                 # a refused load changes nothing
    c.reset()
    assert c.state_dict() == {'tau': 0.25, 'ptilde': [0.25] * 4, 'steps': 0}
    c.load_state_dict({})                       # a checkpoint written before the first update
    assert c.state_dict()['steps'] == 0


def test_config_validation():
    import train
    ce = {'consistency_activation': 'softmax', 'consistency_loss': 'ce'}
    assert train._confidence_threshold_mode({}) == ('fixed', None)
    assert train._confidence_threshold_mode({'confidence_threshold_mode': 'fixed'}) == ('fixed', None)
    assert train._confidence_threshold_mode(dict(ce, confidence_threshold_mode='adaptive')) == ('adaptive', 0.999)
    assert train._confidence_threshold_mode(dict(ce, confidence_threshold_mode='adaptive',
                                                 confidence_threshold_momentum=0)) == ('adaptive', 0.0)
    with pytest.raises(ValueError, match='confidence_threshold_mode'):
        train._confidence_threshold_mode(dict(ce, confidence_threshold_mode='flex'))
    for other in ({}, {'consistency_activation': 'softmax'}, {'consistency_activation': 'softmax',
                                                              'consistency_loss': 'mse'}):
        with pytest.raises(ValueError, match="'ce'"):
            train._confidence_threshold_mode(dict(other, confidence_threshold_mode='adaptive'))
    for bad in (1.0, -0.1, 'high', None, float('nan')):
        with pytest.raises(ValueError, match='confidence_threshold_momentum'):
            train._confidence_threshold_mode(dict(ce, confidence_threshold_mode='adaptive',
                                                  confidence_threshold_momentum=bad))
    # a config without the keys: dictionary lookups only, nothing is created
    tc = dict(ce)
    assert train._adaptive_threshold(tc) is None and tc == ce


def test_the_instance_takes_its_place_in_the_config_and_the_key_components_differ():
    import train
    from ssseg import ops
    ce = {'consistency_activation': 'softmax', 'consistency_loss': 'ce'}
    fixed = dict(ce)
    a = dict(ce, confidence_threshold_mode='adaptive', confidence_threshold_momentum=0.5)
    b = dict(ce, confidence_threshold_mode='adaptive', confidence_threshold_momentum=0.9)
    ka = train._threshold_key(a)
    sat = a['confidence_threshold_state']
    assert isinstance(sat, ops.AdaptiveThreshold) and sat.momentum == 0.5 and train._adaptive_threshold(a) is sat
    assert train._threshold_key(fixed) == ('fixed', None, None) and ka == ('adaptive', 0.5, id(sat))
    kb = train._threshold_key(b)
    assert kb[0] == ka[0] and kb[1] != ka[1] and kb[2] != ka[2]     # another momentum, another state object
    a['confidence_threshold_momentum'] = 0.9                         # one config object, the value changed
    ka2 = train._threshold_key(a)
    assert ka2 == ('adaptive', 0.9, id(sat)) and sat.momentum == 0.9 and ka2 != ka and ka2 != kb
    assert len({ka, kb, ka2, train._threshold_key(fixed)}) == 4
    # an instance the user placed is used as it is
    mine = ops.AdaptiveThreshold(0.1, num_classes=5)
    c = dict(ce, confidence_threshold_mode='adaptive', confidence_threshold_state=mine)
    assert train._adaptive_threshold(c) is mine and mine.momentum == 0.999


def test_train_step_refuses_before_anything_is_launched():
    """the refusal comes before the model's first forward: the model here would raise another error if it were called"""
    import train

    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError('the model was called')
    x = torch.zeros(2, 3, 8, 8)
    ce = {'consistency_activation': 'softmax', 'consistency_loss': 'ce'}
    for bad in (dict(ce, confidence_threshold_mode='flex'), {'confidence_threshold_mode': 'adaptive'},
                dict(ce, confidence_threshold_mode='adaptive', confidence_threshold_momentum=1.0)):
        tc = dict(use_semi_supervised=True, virtual_batch_size_multiplier=1, **bad)
        with pytest.raises(ValueError, match='confidence_threshold'):
            train.train_step(Never(), Never(), None, x, x, x, x, 26, 0, {'train': tc})


def test_new_config_loads_and_selects_the_mode():
    import os
    import config
    import mixmasks
    import train
    here = os.path.join(os.path.dirname(os.path.abspath(config.__file__)), 'configs')
    tc = config.fromfile(os.path.join(here, 'c6_unet_r50_cutmix_ce_adaptive.py'))['train']
    assert mixmasks.mix_mask_kind(tc) == 'cutmix' and train._consistency_loss_kind(tc) == ('ce', 'pixel')
    assert train._confidence_threshold_mode(tc) == ('adaptive', 0.999)
    base = config.fromfile(os.path.join(here, 'c6_unet_r50_cutmix_ce.py'))['train']
    assert train._confidence_threshold_mode(base) == ('fixed', None)
    assert {k for k in tc if k not in base} == {'confidence_threshold_mode', 'confidence_threshold_momentum'}
