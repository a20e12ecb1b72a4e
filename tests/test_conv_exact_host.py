"""Keeps the exact-arithmetic case table (tests/exact.py) honest without a GPU: for every case and regime the GPU file
(test_conv_exact.py) runs, the fp64 reference satisfies the exact-range condition in every compute mode (so
torch.equal against the engine is legitimate: rounding the reference to the storage dtype and back changes nothing)
and the non-degeneracy conditions (so the comparison can see a wrong read)."""
import pytest
import torch

import exact as E


def _all(cases):
    return [pytest.param(c, r, id=f'{c.id}-{r}') for c in cases for r in E.REGIMES]


def _range_all_modes(tensors, shift=0, fp32=E.FP32_OUTPUTS):
    for mode in E.MODES:
        E.check_exact_range(tensors, mode, shift, fp32)
        if mode != 'f32':   # rounding to the storage dtype and back changes nothing
            for name, t in tensors.items():
                if t is not None and name not in fp32:
                    assert torch.equal(t.to(E.TORCH_DTYPE[mode]).double(), t), (name, mode)


@pytest.mark.parametrize('case,regime', _all(E.AUTO_CASES + E.STEM + E.CONVT + E.DEPTHWISE + [E.POINTWISE_SMALL]))
def test_case_is_exact_and_nondegenerate(case, regime):
    ref = E.reference(case, regime)
    _range_all_modes(E.outputs(ref))
    _range_all_modes({k: ref[k] for k in ('x', 'w', 'bias', 'gy')})   # the operands themselves store exactly
    E.nondegenerate(case, ref)


@pytest.mark.parametrize('case,regime', _all(E.MERGED_CASES))
def test_merged_batches_are_exact(case, regime):
    dW = sum(E.reference(case._replace(n=n), regime)['dW'] for n in (2, 3))
    _range_all_modes({'dW': dW})
    assert float((dW != 0).double().mean()) >= 0.25   # (sparse-x: few pixels carry both an activation and a gradient)


@pytest.mark.parametrize('act', E.ACTS, ids=str)
@pytest.mark.parametrize('case,regime', _all(E.ACT_CASES + E.CONVT[:2] + E.DEPTHWISE))
def test_activation_case_is_exact(case, regime, act):
    if (case.kind == 'convT' and act != 'relu') or (case.kind == 'dw' and act != 'relu6'):
        return   # the GPU file runs ConvTranspose2d with ReLU and the depthwise conv with ReLU6 only
    c = E.act_case(case, act)
    ref = E.reference(c, regime, act)
    _range_all_modes(E.outputs(ref), E.act_shift(act))
    y = ref['y']
    # the activation does something and does not kill everything: both branches are taken
    assert 0.15 <= float((y > 0).double().mean()) <= 0.85 or act == E.LEAKY, float((y > 0).double().mean())
    if act == 'relu6':
        assert 0.01 <= float((y == 6).double().mean()) and int((y == 6).sum()) >= 10, 'ReLU6 hardly saturates'
    if act == E.LEAKY:
        assert 0.15 <= float((y < 0).double().mean()) and 0.15 <= float((y > 0).double().mean())
    m = E.reached(c)
    # (the mask closes part of the gradient; a stride-2 depthwise input has two taps)
    assert float((ref['dx'] != 0)[:, :, m].double().mean()) >= 0.25


@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('act', E.CHAIN_ACTS, ids=str)
def test_chain_is_exact(act, regime):
    ref = E.chain_reference(act, regime)
    _range_all_modes({k: ref[k] for k in ('h', 'y', 'dh', 'dx', 'dW1', 'db1', 'dW2')}, E.act_shift(act))
    assert float((ref['y'] != 0).double().mean()) >= 0.5 and float((ref['dx'] != 0).double().mean()) >= 0.5
    assert 0.15 <= float((ref['h'] > 0).double().mean()) <= 0.85


@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('cin,cout,H,W', E.JOIN_CASES)
def test_join_is_exact(cin, cout, H, W, regime):
    ref = E.join_reference(cin, cout, H, W, regime)
    _range_all_modes({k: ref[k] for k in ('z', 'gy', 'add', 'dx')})
    open_ = ref['z'] > 0
    assert 0.2 <= float(open_.double().mean()) <= 0.8
    assert float((ref['dx'] != 0)[open_].double().mean()) >= 0.5


@pytest.mark.parametrize('regime', E.REGIMES)
@pytest.mark.parametrize('ca,cb,H,W', E.VCAT_CASES)
def test_vcat_is_exact(ca, cb, H, W, regime):
    ref = E.vcat_reference(ca, cb, H, W, regime)
    _range_all_modes({k: ref[k] for k in ('y', 'da', 'db_part', 'dW')})
    for k in ('y', 'da', 'db_part'):
        assert float((ref[k] != 0).double().mean()) >= 0.5, k


@pytest.mark.parametrize('case,regime', _all(E.FOLD_CASES))
def test_fold_is_exact(case, regime):
    ref = E.fold_reference(case, regime)
    _range_all_modes({k: ref[k] for k in ('y', 'dx', 'dres', 'dW', 'res')}, shift=1)
    assert set(ref['scale'].tolist()) <= {0.5, 1.0, 2.0} and len(set(ref['scale'].tolist())) > 1
    assert set(ref['var'].tolist()) <= {0.25, 1.0, 4.0} and set(ref['gamma'].tolist()) <= {0.5, 1.0, 2.0}
    assert 0.15 <= float((ref['y'] > 0).double().mean()) <= 0.85
    assert float((ref['dx'] != 0).double().mean()) >= 0.5


@pytest.mark.parametrize('case,regime', _all(E.STATS_CASES))
def test_stats_are_exact(case, regime):
    _range_all_modes(E.stats_reference(case, regime))


def test_operands_are_reproducible():
    """the generators are seeded by text, not by hash(): two builds give the same operands"""
    a = E.conv_operands(E.RAGGED[0], 'sparse-w')
    b = E.conv_operands(E.RAGGED[0], 'sparse-w')
    assert all(torch.equal(s, t) for s, t in zip(a, b) if s is not None)
    x = E.ints((1000,), -2, 2, 0.5, torch.Generator().manual_seed(0))
    assert float(x.min()) >= -2 and float(x.max()) <= 2 and torch.equal(x, x.round())
    assert 0.3 < float((x != 0).double().mean()) < 0.5   # 0.5 kept, a fifth of those drew 0


@pytest.mark.parametrize('mode', ['bf16', 'f16', 'f32'])
def test_one_wrong_element_fails(mode, capsys):
    """What the relative-RMS bound cannot see: one element of 3840 off by one storage step fails assert_exact, and the
    report names it."""
    ref = E.reference(E.CONV_CASES[0], 'sparse-w')
    good = ref['y'].to(E.TORCH_DTYPE[mode])
    assert good.numel() == 3840
    E.assert_exact(good, ref['y'], 'y')
    bad = good.clone()
    bad[1, 5, 7, 3] += 1
    with pytest.raises(AssertionError):
        E.assert_exact(bad, ref['y'], 'y')
    out = capsys.readouterr().out
    assert '1 of 3840 elements differ' in out and '(1, 5, 7, 3)' in out
    rms = float(((bad.double() - ref['y']) ** 2).mean().sqrt() / (ref['y'] ** 2).mean().sqrt())
    assert rms < 2e-2 and rms < 4e-3   # inside both 16-bit bounds of the relative-RMS comparison
