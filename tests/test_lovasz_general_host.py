"""Host-side checks of the general Lovász losses (no GPU): the numpy restatement in tests/lovasz_ref.py reproduces the
reference fixtures (tests/golden/lovasz_gen_*.npz, written by gen_golden_lovasz.py), the C ABI carries the new entry
points, and the public functions validate their arguments and refuse CPU tensors."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import lovasz_ref
from conftest import GOLDEN, golden

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, 'lovasz_gen_*.npz')))
EXPECTED = ['absent_all', 'absent_present', 'hinge_allvoid', 'hinge_batch', 'hinge_image', 'sigmoid', 'sm_all_image',
            'sm_list_image', 'sm_present_batch']


def fixture_call(g):
    """the arguments of a fixture: (x, labels, mode, classes, per_image, ignore)"""
    classes = g['classes']
    classes = str(classes) if classes.dtype.kind == 'U' else [int(c) for c in classes.reshape(-1)]
    ignore = int(g['ignore'])
    return g['x'], g['labels'], str(g['mode']), classes, bool(g['per_image']), None if ignore < 0 else ignore


def test_every_fixture_is_there():
    assert FIXTURES == [f'lovasz_gen_{n}.npz' for n in EXPECTED]


@pytest.mark.parametrize('name', EXPECTED)
def test_ref_reproduces_reference_fixture(name):
    """loss within rtol 1e-5 (fp64 dot against the reference's fp32 torch.dot), gradient within rtol 1e-5 / atol 1e-6:
    the bounds golden G4 uses for the same arithmetic."""
    g = golden(f'lovasz_gen_{name}.npz')
    x, labels, mode, classes, per_image, ignore = fixture_call(g)
    if x.ndim == 3:
        x = x[:, None]
    loss, grad = lovasz_ref.lovasz(x, labels, mode, classes, per_image, ignore)
    np.testing.assert_allclose(loss, float(g['loss']), rtol=1e-5)
    np.testing.assert_allclose(grad.reshape(g['grad'].shape), g['grad'] / np.float32(g['w']), rtol=1e-5, atol=1e-6)


def test_ref_defined_deviations():
    """all-void group: 0 loss, zero gradient, still counted in the mean over groups; one valid pixel: the formula
    (J(0) = 1 - (gts - fg) / (gts + 1 - fg) = 1 either way, so the loss is that pixel's error)."""
    rng = np.random.default_rng(0)
    p = lovasz_ref.softmax(rng.standard_normal((2, 3, 2, 2)).astype(np.float32))
    lab = np.array([[[255, 255], [255, 255]], [[255, 1], [255, 255]]])
    loss, grad = lovasz_ref.lovasz(p, lab, 'probas', [1], True, 255)
    np.testing.assert_allclose(loss, np.float32(1 - p[1, 1, 0, 1]) / 2, rtol=1e-6)
    assert not grad[0].any() and grad[1, 1, 0, 1] == np.float32(-0.5) and np.count_nonzero(grad) == 1
    loss, grad = lovasz_ref.lovasz(p, np.full((2, 2, 2), 255), 'probas', 'all', False, 255)
    assert loss == 0 and not grad.any()


def test_ctypes_table_has_the_general_entry_points():
    from ssseg import native
    lib = native.lib()
    for name in ('ssseg_lovasz_gen_workspace_bytes', 'ssseg_lovasz_gen_fwd', 'ssseg_lovasz_gen_bwd',
                 'ssseg_lovasz_gen_bwd_from_fwd'):
        assert name in native.SIGS and hasattr(lib, name)
    assert lib.ssseg_lovasz_gen_workspace_bytes(2, 3, 35, 1, 3) > 0
    # bounds, checked on the host: C > 64, more than 2^24 pixels per group, groups * classes > 65535
    assert lib.ssseg_lovasz_gen_workspace_bytes(2, 65, 35, 1, 3) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(2, 3, (1 << 24) + 1, 1, 3) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(2, 3, 1 << 24, 0, 3) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1 << 16, 3, 4, 1, 1) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1 << 16, 3, 4, 0, 3) > 0
    one = (ctypes.c_int64 * 1)(1)
    assert lib.ssseg_lovasz_gen_fwd(None, None, 0, 1, 2, 4, 0, 1, 0, one, 1, 0, 0, None, None, 0, None) == -1
    # the workspace of one class chunk does not grow with C: 64 classes against 8 at 4 x 512^2, less the per-pixel
    # weights (4 bytes per class and pixel) that the backward reads
    n = 4 * 512 * 512
    w8 = lib.ssseg_lovasz_gen_workspace_bytes(4, 64, 512 * 512, 1, 8) - 4 * 8 * n
    w64 = lib.ssseg_lovasz_gen_workspace_bytes(4, 64, 512 * 512, 1, 64) - 4 * 64 * n
    assert w64 - w8 < 64 * 4 * 16


def test_functions_refuse_cpu_tensors():
    import lovasz
    import losses
    p = torch.softmax(torch.randn(2, 3, 4, 4), 1)
    lab = torch.randint(0, 3, (2, 4, 4))
    calls = [lambda: lovasz.lovasz_softmax(p, lab), lambda: lovasz.lovasz_softmax(p, lab, classes=[1], per_image=True),
             lambda: lovasz.lovasz_softmax_flat(p[:, :, 0, 0], lab[:, 0, 0]),
             lambda: lovasz.lovasz_hinge(p[:, 0], lab.clamp(max=1)),
             lambda: lovasz.lovasz_hinge_flat(p[:, 0].reshape(-1), lab.clamp(max=1).reshape(-1)),
             lambda: lovasz.binary_xloss(p[:, 0], lab), lambda: lovasz.StableBCELoss()(p, p),
             lambda: losses.LovaszSoftmaxLossWithLogits()(p, p),
             lambda: losses.LovaszHingeLossWithLogits()(p[:, :1], p[:, :1])]
    for call in calls:
        with pytest.raises(RuntimeError, match='HIP device tensor'):
            call()


def test_argument_validation():
    import lovasz
    import losses
    p = torch.rand(2, 4, 4)
    lab = torch.randint(0, 2, (2, 4, 4))
    for classes in ('present', 'all', [0, 1], []):
        with pytest.raises(ValueError):
            lovasz.lovasz_softmax(p, lab, classes=classes)             # C == 1 needs a one-element list
        with pytest.raises(ValueError):
            lovasz.lovasz_softmax(p[:, None], lab, classes=classes)
    p4 = torch.rand(2, 3, 4, 4)
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax(p4, lab[:, :3])                          # labels do not match
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax(p4[0, 0], lab)                           # bad rank
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax(p4, lab, classes=[3])                    # class outside [0, C)
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax(p4, lab, classes='some')
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax(torch.rand(1, 65, 2, 2), lab[:1, :2, :2])   # channel limit
    with pytest.raises(ValueError):
        lovasz.lovasz_softmax_flat(p4, lab)
    with pytest.raises(ValueError):
        lovasz.lovasz_hinge(p4, lab)
    with pytest.raises(ValueError):
        lovasz.lovasz_hinge_flat(p, lab)
    with pytest.raises(NotImplementedError, match='ignore'):
        lovasz.binary_xloss(p, lab, ignore=255)
    with pytest.raises(NotImplementedError, match='labels'):
        lovasz.xloss(p4, lab)
    with pytest.raises(ValueError):
        losses.LovaszSoftmaxLossWithLogits(classes='some')
    with pytest.raises(ValueError):
        losses.LovaszSoftmaxLossWithLogits()(p4[:, :1], p4[:, :1])
    with pytest.raises(ValueError):
        losses.LovaszSoftmaxLossWithLogits()(p4, p4[:, :2])
    with pytest.raises(ValueError):
        losses.LovaszHingeLossWithLogits()(p4, p4)


def test_flatten_helpers_match_their_definition():
    import lovasz
    p = torch.rand(2, 3, 2, 2)
    lab = torch.tensor([[[0, 255], [1, 2]], [[255, 255], [2, 0]]])
    fp, fl = lovasz.flatten_probas(p, lab, 255)
    keep = (lab.reshape(-1) != 255)
    assert torch.equal(fl, lab.reshape(-1)[keep])
    assert torch.equal(fp, p.permute(0, 2, 3, 1).reshape(-1, 3)[keep])
    fs, fl2 = lovasz.flatten_binary_scores(p[:, 0], lab, 255)
    assert torch.equal(fs, p[:, 0].reshape(-1)[keep]) and torch.equal(fl2, fl)
    fp, fl = lovasz.flatten_probas(p[:, 0], lab)
    assert fp.shape == (8, 1) and fl.shape == (8,)
