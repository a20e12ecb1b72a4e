"""Host-side checks of the ClassMix / CutMix masks: the CPU restatements (tests/mixmask_ref.py) against hand-worked
cases, the box geometry's edge cases and area bound, the config key, and the C entry points' argument validation
(no device is touched)."""
import ctypes

import pytest
import torch

import mixmask_ref as R

SHAPES = ((17, 31), (64, 48), (130, 127))


def _one_hot_logits(lab, C):
    """[B,H,W] labels -> logits [B,C,H,W] whose argmax they are"""
    return torch.nn.functional.one_hot(torch.as_tensor(lab), C).permute(0, 3, 1, 2).float()


def test_classmix_known_subset_at_three_classes():
    # labels: class 0 on row 0, class 1 on row 1, class 2 on row 2; keys 50, 10, 30 -> order 1, 2, 0; k = ceil(3/2) = 2
    lab = torch.tensor([[[0, 0], [1, 1], [2, 2]]])
    mask, present, chosen, n, k = R.classmix(_one_hot_logits(lab, 3), torch.tensor([[50, 10, 30]]))
    print('present', R.fmt_words(present), 'chosen', R.fmt_words(chosen), 'n', n, 'k', k, 'mask', mask.flatten().tolist())
    assert n == [3] and k == [2]
    assert present.tolist() == [0b111] and chosen.tolist() == [0b110]
    assert torch.equal(mask, torch.tensor([[0., 0.], [1., 1.], [1., 1.]]).view(1, 1, 3, 2))


def test_classmix_single_class_gives_a_full_mask():
    lab = torch.full((1, 3, 2), 2)
    mask, present, chosen, n, k = R.classmix(_one_hot_logits(lab, 4), torch.tensor([[1, 2, 3, 4]]))
    print('present', R.fmt_words(present), 'chosen', R.fmt_words(chosen), 'n', n, 'k', k)
    assert n == [1] and k == [1] and present.tolist() == [0b100] and chosen.tolist() == [0b100]
    assert torch.equal(mask, torch.ones(1, 1, 3, 2))


def test_classmix_key_tie_goes_to_the_lower_class():
    # four classes present, all keys equal: (key, c) orders them by class index, k = 2 -> classes 0 and 1
    lab = torch.tensor([[[0, 1], [2, 3]]])
    mask, _, chosen, n, k = R.classmix(_one_hot_logits(lab, 4), torch.tensor([[7, 7, 7, 7]]))
    print('chosen', R.fmt_words(chosen), 'n', n, 'k', k)
    assert n == [4] and k == [2] and chosen.tolist() == [0b0011]
    assert torch.equal(mask, torch.tensor([[1., 1.], [0., 0.]]).view(1, 1, 2, 2))
    # a tie between an absent class with the same key and a present one never picks the absent class
    lab = torch.tensor([[[1, 1], [3, 3]]])
    _, present, chosen, n, k = R.classmix(_one_hot_logits(lab, 4), torch.tensor([[7, 7, 7, 7]]))
    assert present.tolist() == [0b1010] and chosen.tolist() == [0b0010] and (n, k) == ([2], [1])


def test_labels_first_maximum_and_nan():
    x = torch.tensor([[1., 1., 0.], [0., 2., 2.], [0., float('nan'), 5.], [float('nan'), float('nan'), 9.],
                      [3., 1., float('nan')]]).t().reshape(1, 3, 1, 5)
    lab = R.labels(x)
    print('labels', lab.flatten().tolist())
    assert lab.flatten().tolist() == [0, 1, 1, 0, 2]
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 7, 5, 6, generator=g)
    assert torch.equal(R.labels(y), y.argmax(1))


def test_designed_classmix_inputs_cover_the_cases():
    full = odd = one = False
    for C in (1, 2, 3, 19, 33, 64, 4, 5, 8, 9, 16, 17, 32):
        for H, W in ((17, 31), (7, 9)):
            x, keys = R.classmix_inputs(C, H, W)
            _, _, _, n, k = R.classmix(x, keys)
            full |= any(v == C for v in n)
            odd |= any(v % 2 == 1 and v > 1 for v in n)
            one |= any(v == 1 for v in n)
            assert all(kk == (nn + 1) // 2 for nn, kk in zip(n, k))
    print('every class present', full, 'odd n', odd, 'n = 1', one)
    assert full and odd and one


@pytest.mark.parametrize('H,W', SHAPES)
def test_box_edges(H, W):
    ones = torch.tensor([[0.3, 0.6, 0.2, 0.9]])
    mask, boxes = R.cutmix(ones, H, W, (1.0, 1.0))            # p = 1: the full mask
    print('p = 1', boxes.tolist())
    assert boxes.tolist() == [[0, 0, H, W]] and bool(mask.all())
    mask, boxes = R.cutmix(ones, H, W, (0.0, 0.0))            # p = 0, u > 0: h = 0, the empty mask
    print('p = 0', boxes.tolist())
    assert boxes[0, 2] == 0 and not bool(mask.any())
    tiny = torch.tensor([[0.0, R.ONE, 0.5, 0.5]])             # H p^u < 0.5 at p = 1e-3: h = 0 with w = W
    mask, boxes = R.cutmix(tiny, H, W, (1e-3, 1e-3))
    print('tiny p', boxes.tolist())
    assert boxes[0, 2] == 0 and boxes[0, 3] == W and not bool(mask.any())
    mask, boxes = R.cutmix(R.DESIGNED, H, W, R.RANGE)
    print('designed', boxes.tolist())
    b = boxes.tolist()
    assert b[1][:2] == [0, 0]                                                  # v = 0: flush to the top-left
    assert b[2][0] + b[2][2] == H and b[2][1] + b[2][3] == W                   # v -> 1: flush to the bottom-right
    assert b[3][2] == H and b[4][3] == W                                       # u = 0 / u -> 1: full bands
    assert b[5][0] + b[5][2] == H and b[5][1] == 0 and b[6][0] == 0 and b[6][1] + b[6][3] == W
    for (top, left, h, w), m in zip(b, mask):
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W
        assert int(m.sum()) == h * w and bool(m[0, top:top + h, left:left + w].all())


@pytest.mark.parametrize('H,W', SHAPES)
def test_box_area_bound_and_rounding_margin(H, W):
    p, th, tw, tt, tl = R.cutmix_terms(R.DESIGNED, H, W, R.RANGE)
    margin = min(float(R.half_integer_distance(t).min()) for t in (th, tw, tt, tl))
    gaps = R.area_gaps(R.cutmix_boxes(R.DESIGNED, H, W, R.RANGE), p, H, W)
    print('distance to a half-integer', margin, 'area gaps', gaps)
    assert margin >= 1e-6
    assert all(err <= bound for err, bound in gaps)


def test_half_to_even():
    # p = 0.25, u = 0.5: p^u = 0.5 exactly, so H p^u = 2.5 at H = 5 and 3.5 at H = 7: rint -> 2 and 4
    q = torch.tensor([[0.0, 0.5, 0.0, 0.0]])
    assert R.cutmix_boxes(q, 5, 7, (0.25, 0.25))[0, 2] == 2 and R.cutmix_boxes(q, 7, 5, (0.25, 0.25))[0, 2] == 4


def test_unknown_mix_mask_is_refused():
    import mixmasks
    import train
    assert mixmasks.mix_mask_kind({}) == 'cowmix'
    for kind in ('cowmix', 'cutmix', 'classmix'):
        assert mixmasks.mix_mask_kind({'mix_mask': kind}) == kind
    with pytest.raises(ValueError, match='mix_mask'):
        mixmasks.mix_mask_kind({'mix_mask': 'fmix'})
    # the step refuses it before the model or any kernel is touched: the model here would raise something else
    tc = dict(use_semi_supervised=True, mix_mask='fmix')
    with pytest.raises(ValueError, match='mix_mask'):
        train.train_step(None, None, None, None, None, None, None, 26, 0, {'train': tc})


def test_draw_sources_on_the_host():
    import mixmasks
    with pytest.raises(ValueError, match='keys'):
        mixmasks.set_draws(keys=torch.tensor([[-1, 2]]))
    with pytest.raises(ValueError, match='params'):
        mixmasks.set_draws(params=torch.ones(2, 4))
    try:
        mixmasks.set_draws(keys=torch.tensor([[3, 1, 2 ** 31 - 1]], dtype=torch.int32))
        assert mixmasks.draws_fixed() and not mixmasks.capturable('classmix') and mixmasks.capturable('cowmix')
    finally:
        mixmasks.set_draws()
    assert not mixmasks.draws_fixed() and mixmasks.capturable('classmix')
    assert mixmasks.counter_advance(4096, 4) == 8192 and mixmasks.counter_advance(2, 19) == 12
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        from ssseg import ops
        ops.classmix_mask(x, torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        ops.cutmix_mask(torch.zeros(2, 4), 4, 4, (0.25, 0.75))


def test_entry_points_validate_on_the_host():
    from ssseg import native
    lib = native.lib()
    st = (ctypes.c_int64 * 4)(48, 16, 4, 1)
    one = ctypes.c_void_p(16)      # a non-null pointer that must never be dereferenced
    f = lib.ssseg_classmix_mask
    rc = {
        'null logits': f(None, st, 0, one, 1, 3, 4, 4, one, None, None, one, 1 << 20, None),
        'null strides': f(one, None, 0, one, 1, 3, 4, 4, one, None, None, one, 1 << 20, None),
        'null keys': f(one, st, 0, None, 1, 3, 4, 4, one, None, None, one, 1 << 20, None),
        'null mask': f(one, st, 0, one, 1, 3, 4, 4, None, None, None, one, 1 << 20, None),
        'C = 0': f(one, st, 0, one, 1, 0, 4, 4, one, None, None, one, 1 << 20, None),
        'C = 65': f(one, st, 0, one, 1, 65, 4, 4, one, None, None, one, 1 << 20, None),
        'B < 0': f(one, st, 0, one, -1, 3, 4, 4, one, None, None, one, 1 << 20, None),
        'H < 0': f(one, st, 0, one, 1, 3, -4, 4, one, None, None, one, 1 << 20, None),
        'cutmix null params': lib.ssseg_cutmix_mask(None, 1, 4, 4, 0.25, 0.75, one, None, None),
        'cutmix null mask': lib.ssseg_cutmix_mask(one, 1, 4, 4, 0.25, 0.75, None, None, None),
        'cutmix W < 0': lib.ssseg_cutmix_mask(one, 1, 4, -4, 0.25, 0.75, one, None, None),
        'draw no output': lib.ssseg_mixmask_draw_dev(None, None, 2, 3, 1, one, None),
        'draw null counter': lib.ssseg_mixmask_draw_dev(one, one, 2, 3, 1, None, None),
        'draw C = 0': lib.ssseg_mixmask_draw_dev(one, one, 2, 0, 1, one, None),
        'draw C = 65': lib.ssseg_mixmask_draw_dev(one, one, 2, 65, 1, one, None),
    }
    print(rc)
    assert all(v == -1 for v in rc.values()), rc
    need = lib.ssseg_classmix_workspace_bytes(16, 512, 512)
    print('workspace bytes', need)
    assert need >= 16 * 512 * 512
    assert f(one, st, 0, one, 1, 3, 4, 4, one, None, None, None, 0, None) == -3      # no workspace: SSSEG_EWORKSPACE
