"""Host side of the fused parameter step (ssseg.param_step): the descriptor grouping and the eligibility rule.  No
device: group() is pure Python and eligible() only looks at the objects it is given."""
import types

import pytest
import torch

import param_step_cases as cases
from ssseg import optim, param_step


def _weights(order=None):
    slots, numel = cases.layout()
    ws = [(off, shape, [(1000 * (i + 1) + j, t, spec) for j, (t, spec) in enumerate(packs)])
          for i, (_, off, _, shape, packs) in enumerate(slots) if shape is not None]
    return (ws if order is None else [ws[i] for i in order]), numel


def test_group_covers_the_arena_once_and_keys_by_weight():
    ws, numel = _weights(order=[2, 0, 3, 1])   # any order in: sorted by offset out
    descs, packs = param_step.group(numel, ws)
    assert all(len(d) == param_step.DESC_WORDS for d in descs) and all(len(p) == param_step.PACK_WORDS for p in packs)
    pos = 0
    for off, n, *_ in descs:      # contiguous, no overlap, no hole
        assert off == pos and n > 0
        pos += n
    assert pos == numel
    conv = [d for d in descs if d[2] != 0]
    flat = [d for d in descs if d[2] == 0]
    # ONE descriptor per master weight however many packs and layouts it has
    assert [(d[2], d[3], d[4], d[5]) for d in conv] == [(8, 8, 1, 1), (64, 8, 7, 7), (72, 40, 3, 3), (24, 16, 4, 4)]
    assert [d[9] for d in conv] == [1, 2, 4, 10] and [d[8] for d in conv] == [0, 1, 3, 7]
    assert len(packs) == 17 and len({p[0] for p in packs}) == 17
    # the gaps: 1, 255, 1027 and 5 elements plus the alignment of the slot before each
    assert [d[1] for d in flat] == [4, 256, 1028, 8]
    # padded extents: w3 has a pack with 80 rows x 48 channels, wT a 20-channel layout-0 pack
    assert (conv[2][6], conv[2][7]) == (80, 48) and (conv[3][6], conv[3][7]) == (24, 20)
    assert (conv[1][6], conv[1][7]) == (64, 8)
    # student / teacher flags survive; layout-1 packs keep their own Kd / Cp
    w3 = packs[3:7]
    assert [p[1] for p in w3] == [0, 0, 0, 1] and [p[2] for p in w3] == [0, 0, 1, 0]
    assert (w3[2][3], w3[2][4]) == (40, 72)


def test_group_without_weights_is_one_range():
    assert param_step.group(64, []) == ([(0, 64, 0, 0, 0, 0, 0, 0, 0, 0)], [])


@pytest.mark.parametrize('mutate,match', [
    ('overlap', 'overlaps'), ('unaligned', 'aligned'), ('taps', 'taps'), ('spec', 'does not describe'),
    ('nopacks', 'packs'), ('numel', 'multiple of 4'), ('outside', 'leaves the arena')])
def test_group_refuses_what_the_kernel_cannot_take(mutate, match):
    ws, numel = _weights()
    if mutate == 'overlap':
        ws[1] = (ws[0][0] + 4,) + ws[1][1:]
    elif mutate == 'unaligned':
        ws[0] = (2,) + ws[0][1:]
    elif mutate == 'taps':
        ws[0] = (ws[0][0], (1, 1, 12, 12), [(1, 0, (1, 1, 1, 12, 12, 8, 0, 0, 1, 12, 0, 1, 12))])
    elif mutate == 'spec':   # a layout-1 spec on a weight whose extents are the other way round
        ws[1] = ws[1][:2] + ([(1, 0, (64, 64, 8, 7, 7, 8, 1, 0, 1, 7, 0, 1, 7))],)
    elif mutate == 'nopacks':
        ws[0] = ws[0][:2] + ([],)
    elif mutate == 'numel':
        numel += 2
    elif mutate == 'outside':
        numel = ws[-1][0] + 8
    with pytest.raises(ValueError, match=match):
        param_step.group(numel, ws)


class _Arena:
    def __init__(self, shapes=((3, 3), (5,)), grads=True, dtype=torch.float32):
        self.numel = 16
        self.shapes = shapes
        self.data = types.SimpleNamespace(is_cuda=True, dtype=dtype, device='cuda:0')
        self.grad = object() if grads else None

    def compatible(self, other):
        return self.shapes == other.shapes


def _sgd(arena, scaler=None, cls=optim.SGD):
    o = cls.__new__(cls)
    o.arena, o.grad_scaler = arena, scaler
    return o


def test_eligibility_rule(monkeypatch):
    monkeypatch.delenv('SSSEG_PARAM_STEP', raising=False)
    s, t = _Arena(), _Arena(grads=False)
    assert param_step.eligible(s, t, _sgd(s))
    for why, args in [
        ('not plain SGD', (s, t, _sgd(s, cls=optim.Adam))),
        ('not plain SGD', (s, t, _sgd(s, cls=type('Sub', (optim.SGD,), {})))),
        ('loss-scaled', (s, t, _sgd(s, scaler=object()))),
        ('no flat arena', (s, None, _sgd(s))),
        ('no flat arena', (None, t, _sgd(s))),
        ('no flat arena', (s, t, _sgd(_Arena()))),            # the optimizer steps another arena
        ('without gradients', (_Arena(grads=False), t, None)),
        ('not fp32', (s, _Arena(dtype=torch.bfloat16), _sgd(s))),
        ('arenas differ', (s, _Arena(shapes=((3, 3),)), _sgd(s))),
    ]:
        a, b, o = args
        o = o if o is not None else _sgd(a)
        reasons = []
        assert not param_step.eligible(a, b, o, reasons), why
        assert len(reasons) == 1 and why in reasons[0], (why, reasons)
    monkeypatch.setenv('SSSEG_PARAM_STEP', '0')
    reasons = []
    assert not param_step.eligible(s, t, _sgd(s), reasons) and reasons == ['SSSEG_PARAM_STEP=0']
