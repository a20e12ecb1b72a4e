"""CPU: the fp64 restatements of tests/multiclass_ref.py against direct torch expressions and the reference's recorded
lovasz.iou values, the C-class synthetic dataset, and the new C ABI symbols."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as R
from conftest import golden


@pytest.mark.parametrize('C', [2, 3, 19])
def test_consistency_restatement(C):
    g = torch.Generator().manual_seed(C)
    s = torch.randn(2, C, 7, 9, generator=g, dtype=torch.float64)
    t = 3 * torch.randn(2, C, 7, 9, generator=g, dtype=torch.float64)
    w = torch.rand(2, 7, 9, generator=g, dtype=torch.float64)
    thr = 0.6
    # written out per pixel, without torch.softmax
    es, et = torch.exp(s - s.amax(1, keepdim=True)), torch.exp(t - t.amax(1, keepdim=True))
    ps, pt = es / es.sum(1, keepdim=True), et / et.sum(1, keepdim=True)
    for weight in (None, w):
        cm = (pt.amax(1) > thr).double() * (1.0 if weight is None else weight)
        want = (((ps - pt) ** 2).sum(1) * cm).sum() / cm.sum()
        loss, cm_mean, cnt = R.consistency_softmax(s, t, thr, weight)
        assert 0 < float(cm.sum()) < cm.numel()
        assert torch.allclose(loss, want, rtol=1e-13, atol=0) and torch.allclose(cnt, cm.sum(), rtol=1e-13)
        assert torch.allclose(cm_mean, cm.mean(), rtol=1e-13)
        # the analytic gradient of the header: 2 cm / sum(cm) * ps_c (d_c - sum_k d_k ps_k)
        _, _, _, grad = R.consistency_softmax_grad(s, t, thr, weight, gout=0.7)
        d = ps - pt
        want_g = 2 * 0.7 * (cm / cm.sum()).unsqueeze(1) * ps * (d - (d * ps).sum(1, keepdim=True))
        assert np.allclose(grad, want_g.numpy(), rtol=1e-11, atol=1e-16)
    # the sigmoid form is another loss (what the mutated-copy test of test_multiclass.py relies on)
    assert not torch.allclose(R.consistency_softmax(s, t, thr, activation='sigmoid')[0],
                              R.consistency_softmax(s, t, thr)[0], rtol=1e-3)


@pytest.mark.parametrize('C', [1, 2, 3, 19, 64])
def test_confident_teacher_design(C):
    thr = 0.7
    for scale in (1.0, 1e4):
        t, conf = R.confident_teacher((2, C, 7, 9), thr, seed=C, scale=scale)
        p = torch.softmax(t.double(), 1).amax(1)
        assert torch.isfinite(p).all() and float((p - thr).abs().min()) >= 1e-3
        assert torch.equal(p > thr, conf)
        if C > 1:
            assert 0 < int(conf.sum()) < conf.numel()


@pytest.mark.parametrize('C', [2, 3, 19])
def test_metrics_restatement(C):
    g = torch.Generator().manual_seed(100 + C)
    logits = torch.randn(3, C, 6, 5, generator=g)
    label = torch.randint(0, C, (3, 12, 10), generator=g)
    mask = F.one_hot(label, C).permute(0, 3, 1, 2).float()
    m = R.seg_metrics(logits, mask)
    # train.py:171-175 written out with num_classes = C
    one_hot = F.one_hot(torch.argmax(logits, dim=1), num_classes=C).permute(dims=(0, 3, 1, 2)).to(logits)
    pred_bin = F.interpolate(one_hot, size=mask.size()[2:4], mode='nearest')
    mask_bin = (mask > 0.5).to(mask)
    a, b = pred_bin[:, 1:].double(), mask_bin[:, 1:].double()
    dice = (2. * (a * b).sum(dim=(1, 2, 3)) + 1.) / ((a + b).sum(dim=(1, 2, 3)) + 1.)
    assert abs(m['dice_mean'] - float(dice.mean())) < 1e-14
    pred = pred_bin.argmax(1)
    assert np.allclose(m['ious'], R.iou(pred, label, C), rtol=0, atol=1e-15)
    assert int(m['conf'].sum()) == label.numel() and torch.equal(m['conf'].sum(1), torch.bincount(label.flatten(),
                                                                                                  minlength=C))
    # the label-map form counts the same, and an ignore value takes its pixels out of every count
    ml = R.seg_metrics(logits, label)
    assert torch.equal(ml['conf'], m['conf']) and torch.equal(ml['dice'], m['dice'])
    lab_i = label.clone()
    lab_i[:, ::3] = 255
    mi = R.seg_metrics(logits, lab_i, ignore=255)
    assert int(mi['conf'].sum()) == int((lab_i != 255).sum())
    assert np.allclose(mi['ious'], R.iou(pred, lab_i, C, ignore=255), rtol=0, atol=1e-15)
    # a running total
    m2 = R.seg_metrics(logits, mask, total=m['conf'])
    assert np.allclose(m2['ious'], m['ious'], rtol=0, atol=1e-15)


def test_iou_matches_the_reference_fixture():
    z = golden('multiclass_iou.npz')
    names = sorted({k.split('.')[0] for k in z.files if '.' in k})
    assert names == ['c19', 'c19_ignore', 'c2', 'c3', 'c5_absent']
    for n in names:
        C, ignore = int(z[f'{n}.C']), int(z[f'{n}.ignore'])
        ignore = None if ignore < 0 else ignore
        pred, label = torch.from_numpy(z[f'{n}.pred']), torch.from_numpy(z[f'{n}.label'])
        want = z[f'{n}.iou100']
        assert np.allclose(100 * R.iou(pred, label, C, ignore), want, rtol=1e-14, atol=0), n
        # and through the confusion matrix, the way the kernel and train.validate take it
        conf = R.confusion(pred, label, C, ignore).double()
        i = conf.diagonal()
        u = conf.sum(0) + conf.sum(1) - i
        got = torch.where(u > 0, i / u.clamp(min=1), torch.ones_like(i)).numpy()
        assert np.allclose(100 * got, want, rtol=1e-14, atol=0), n
    assert z['c5_absent.iou100'][3] == 100.0


def test_prob_onehot_restatement():
    x = torch.tensor([[[[1.0, 2.0]], [[1.0, float('nan')]], [[0.5, 3.0]]]])    # [1,3,1,2]: a tie, a NaN
    for act in ('sigmoid', 'softmax'):
        prob, onehot = R.prob_onehot(x, act)
        assert onehot[0, :, 0, 0].tolist() == [1.0, 0.0, 0.0]      # the first maximum
        assert onehot[0, :, 0, 1].tolist() == [0.0, 1.0, 0.0]      # NaN is the maximum
    assert torch.allclose(R.prob_onehot(x, 'softmax')[0][0, :, 0, 0].sum(), torch.tensor(1.0, dtype=torch.float64))


def test_synthetic_dataset_classes():
    from data.synthetic import SyntheticSegDataset
    a = SyntheticSegDataset(length=2, size=48, seed=5, blob_sigma=3.0)
    b = SyntheticSegDataset(length=2, size=48, seed=5, blob_sigma=3.0, num_classes=2)
    for i in range(2):
        for k in ('image', 'semantic_mask'):
            assert torch.equal(a[i][k], b[i][k]) and a[i][k].dtype == b[i][k].dtype
    assert a[0]['semantic_mask'].shape == (2, 48, 48)
    d = SyntheticSegDataset(length=2, size=48, seed=5, blob_sigma=3.0, num_classes=5)
    m = d[1]['semantic_mask']
    assert m.shape == (5, 48, 48) and m.dtype == torch.float32
    assert torch.equal(m.sum(0), torch.ones(48, 48)) and set(m.unique().tolist()) == {0.0, 1.0}
    assert all(float(m[c].sum()) > 0 for c in range(5))
    assert torch.equal(d[1]['image'], a[1]['image'])               # the image does not depend on the class count
    assert torch.equal(d[1]['semantic_mask'], d[1]['semantic_mask'])
    with pytest.raises(ValueError):
        SyntheticSegDataset(num_classes=1)


def test_header_declares_the_multiclass_entry_points():
    from ssseg import native
    declared = set(native.header_symbols())
    new = {'ssseg_consistency_sm_fwd', 'ssseg_consistency_sm_bwd', 'ssseg_seg_metrics_mc', 'ssseg_prob_onehot_mc'}
    assert new <= declared and new <= set(native.SIGS)
    lib = native.lib()
    # argument errors are detected on the host: null pointers and 65 channels -> SSSEG_EINVAL
    assert lib.ssseg_consistency_sm_fwd(None, None, None, 1, 3, 8, 0.5, None, None, 0, None) == -1
    assert lib.ssseg_consistency_sm_bwd(None, None, None, 1, 3, 8, 0.5, None, None, None, None) == -1
    assert lib.ssseg_prob_onehot_mc(None, 1, 3, 8, 1, None, None, None) == -1
    one = torch.zeros(1)
    p = one.data_ptr()     # never dereferenced: the channel count is refused first
    assert lib.ssseg_consistency_sm_fwd(p, p, None, 1, 65, 8, 0.5, p, p, 1 << 20, None) == -1
    assert lib.ssseg_prob_onehot_mc(p, 1, 65, 8, 0, p, p, None) == -1
    assert lib.ssseg_prob_onehot_mc(p, 1, 3, 8, 2, p, p, None) == -1
    # a workspace smaller than ssseg_reduce_workspace_bytes -> SSSEG_EWORKSPACE
    assert lib.ssseg_consistency_sm_fwd(p, p, None, 1, 3, 8, 0.5, p, p, 8, None) == -3


def test_ops_refuse_bad_arguments():
    from ssseg import ops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.consistency_loss_softmax(x, x, 0.5)
    with pytest.raises(ValueError, match='65 channels'):
        ops.consistency_loss_softmax(torch.zeros(1, 65, 2, 2), torch.zeros(1, 65, 2, 2), 0.5)
    with pytest.raises(ValueError, match='one shape'):
        ops.consistency_loss_softmax(x, torch.zeros(2, 3, 4, 5), 0.5)
    with pytest.raises(ValueError, match='one weight per pixel'):
        ops.consistency_loss_softmax(x, x, 0.5, torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match='65 channels'):
        ops.SegMetricsMC('cpu', 65)
    with pytest.raises(ValueError, match='65 channels'):
        ops.prob_onehot(torch.zeros(1, 65, 2, 2))
    with pytest.raises(ValueError, match='activation'):
        ops.prob_onehot(x, 'tanh')
    with pytest.raises(ValueError, match='HIP device tensor'):
        ops.prob_onehot(x, 'softmax')
