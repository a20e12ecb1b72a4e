"""GPU: ssseg.active.score_pool / partition on a synthetic pool of 20 images at 64x64 in batches of 8 (the last batch
holds 4): rows in loader order and independent of the batching, features against the plain mean, a submodule as the
feature source, and the whole partition against active_ref on the returned scores and features."""
import numpy as np
import pytest
import torch

import active_ref as R

pytestmark = pytest.mark.gpu

POOL, BATCH, SIZE = 20, 8, 64


@pytest.fixture
def f32_mode():
    from ssseg import nn as snn
    snn.set_compute_dtype(torch.float32)
    yield
    snn.set_compute_dtype(torch.bfloat16)


def _pool():
    from data.synthetic import SyntheticSegDataset
    return SyntheticSegDataset(length=POOL, size=SIZE, seed=5, with_masks=False)


def _loader(batch=BATCH):
    return torch.utils.data.DataLoader(_pool(), batch_size=batch, shuffle=False)


def _simple_unet(dev, classes=3):
    from models import simple_unet
    from models.adapters import ListOutput
    torch.manual_seed(0)
    net = simple_unet.UNet(classes, num_blocks=2, first_channels=8, max_width=32)
    # an untrained net in eval mode (BatchNorm at its initial statistics) gives logits of some 1e-4, every image
    # scoring log C: scale the head so that the logits are of order 1 and the images differ
    with torch.no_grad():
        net.final_block[1].weight.mul_(2e4)
    return ListOutput(net).to(dev).eval()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_score_pool_rows_and_features(hip_device):
    from ssseg import active, ops
    model = _simple_unet(hip_device)
    model.train()
    scores, feats = active.score_pool(model, _loader())
    assert model.training                                              # the mode is restored
    model.eval()
    assert scores.shape == (POOL, 3) and scores.dtype == torch.float32 and scores.is_cuda
    assert feats.shape == (POOL, 3) and feats.dtype == torch.float32 and feats.is_cuda
    rows, means, mags = [], [], []
    with torch.no_grad():
        for batch in _loader():
            f, logits = model(batch['image'].to(hip_device))
            for b in range(logits[-1].shape[0]):                       # every image's logits scored alone
                rows.append(ops.uncertainty_scores(logits[-1][b:b + 1]))
            means.append(f[-1].double().mean((2, 3)))
            mags.append(f[-1].double().abs().mean((2, 3)))
    assert np.array_equal(_bits(scores), _bits(torch.cat(rows)))
    # the pooling kernel reads the logits rounded to bf16 and rounds its mean to bf16: 2 x 2^-9 of the mean magnitude
    err = (feats.double() - torch.cat(means)).abs()
    bound = 2.0 ** -8 * torch.cat(mags) * 1.01 + 1e-7
    print('feature error', float(err.max()), 'bound', float(bound.min()))
    assert bool((err <= bound).all())
    # another batching of the same pool: the same scores up to the model's own batch dependence (none is expected
    # beyond rounding), the same order
    s1, _ = active.score_pool(model, _loader(batch=1))
    print('batch 8 against batch 1', float((s1 - scores).abs().max()))
    assert float((s1 - scores).abs().max()) <= 2e-2 * float(scores.abs().max())
    assert not model.training


def test_feature_source_submodule(hip_device):
    from models import unet
    from models.adapters import ListOutput
    from models.encoders import mobilenetv2
    from ssseg import active
    torch.manual_seed(1)
    model = ListOutput(unet.UNet(2, mobilenetv2.mobilenet_v2(width_mult=0.35), 32, train_upsampling=True)).to(
        hip_device).eval()
    width = model.model.encoder.endpoint_depths[-1]
    captured = []
    h = model.model.encoder.register_forward_hook(lambda m, i, o: captured.append(o[-1]))
    scores, feats = active.score_pool(model, _loader(), feature_source='encoder')
    h.remove()
    assert scores.shape == (POOL, 3)
    assert feats.shape == (POOL, width)
    want = torch.cat([c.double().mean((2, 3))[:, :width] for c in captured])
    mag = torch.cat([c.double().abs().mean((2, 3))[:, :width] for c in captured])
    err = (feats.double() - want).abs()
    print('encoder feature error', float(err.max()))
    assert bool((err <= 2.0 ** -9 * mag * 1.01 + 1e-6).all())          # one bf16 rounding of the mean
    assert len(model.model.encoder._forward_hooks) == 0                # score_pool removed its hook
    with pytest.raises(ValueError, match='feature_source'):
        active.score_pool(model, _loader(), feature_source='no_such_module')
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        active.score_pool(model, _loader(), device='cpu')


def test_partition_agrees_with_the_oracle(hip_device, f32_mode):
    from ssseg import active
    model = _simple_unet(hip_device)
    kw = dict(num_clusters=3, per_cluster=2, seed=11, feature_source='encoder.2.1')
    a = active.partition(model, _loader(), **kw)
    b = active.partition(model, _loader(), **kw)
    assert a['clusters'] == b['clusters'] and a['ranking'] == b['ranking']
    assert np.array_equal(a['labels'].cpu().numpy(), b['labels'].cpu().numpy())
    assert a['centroids'].cpu().numpy().tobytes() == b['centroids'].cpu().numpy().tobytes()
    assert len(a['clusters']) == 3
    chosen = [i for c in a['clusters'] for i in c]
    assert all(len(c) <= 2 for c in a['clusters']) and len(set(chosen)) == len(chosen)
    assert all(0 <= i < POOL for i in chosen) and sorted(a['ranking']) == list(range(POOL))
    assert a['features'].shape == (POOL, 32)
    # the oracle on the returned scores and features, the uniforms drawn as partition draws them
    u = torch.rand(3, generator=torch.Generator().manual_seed(11)).numpy()
    o = R.kmeans(a['features'].cpu().numpy(), 3, u=u)
    print('oracle gaps', o['gap'], o['seed_gap'], 'n_iter', o['n_iter'])
    assert o['gap'] >= 1e-9 and o['seed_gap'] >= 1e-9
    assert np.array_equal(a['seed_idx'].cpu().numpy(), o['seed_idx'])
    assert np.array_equal(a['labels'].cpu().numpy(), o['labels']) and int(a['n_iter']) == o['n_iter']
    s = a['scores'].cpu().numpy()
    assert a['clusters'] == R.select(s[:, 0], o['labels'], 2, 3) and a['ranking'] == R.rank(s[:, 0])
    # n_init > 1: the lowest inertia of the fits drawn from the same generator
    c = active.partition(model, _loader(), n_init=3, **kw)
    g = torch.Generator().manual_seed(11)
    fits = [R.kmeans(a['features'].cpu().numpy(), 3, u=torch.rand(3, generator=g).numpy()) for _ in range(3)]
    best = min(fits, key=lambda f: f['inertia'])
    assert np.array_equal(c['labels'].cpu().numpy(), best['labels'])
    np.testing.assert_allclose(float(c['inertia']), best['inertia'], rtol=1e-9)


def test_entry_point_end_to_end(hip_device, tmp_path):
    """a checkpoint, a directory of JPEGs of mixed sizes and a config with an active_learning dict -> the JSON document"""
    import json

    from PIL import Image

    import get_active_learning_partition as cli
    rng = np.random.default_rng(9)
    pool = tmp_path / 'pool'
    pool.mkdir()
    for i in range(13):
        h, w = (48, 64) if i % 2 else (64, 40)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(pool / f'img_{i:02d}.jpg')
    cfg = tmp_path / 'al_e2e_cfg.py'
    cfg.write_text("from models import simple_unet\nfrom models.adapters import ListOutput\n"
                   "common = dict(image_size=64)\n"
                   "model = dict(model_fn=lambda: ListOutput(simple_unet.UNet(3, num_blocks=2, first_channels=8, "
                   "max_width=32)))\n"
                   "active_learning = dict(num_clusters=3, per_cluster=2, feature_source='encoder.2.1', batch_size=4)\n")
    student, teacher = _simple_unet('cpu'), _simple_unet('cpu')
    with torch.no_grad():
        for p in teacher.parameters():
            p.mul_(0.5)
    ck = tmp_path / 'ck.pth'
    torch.save({'epoch': 1, 'best_metric': 0.0, 'state_dict': student.state_dict(),
                'ema_state_dict': teacher.state_dict()}, ck)
    docs = {}
    for weights in ('ema', 'student'):
        out = tmp_path / f'{weights}.json'
        cli.main([str(cfg), '--checkpoint', str(ck), '--images', str(pool), '--weights', weights, '--score', 'margin',
                  '--seed', '4', '--out', str(out)])
        docs[weights] = json.loads(out.read_text())
    d = docs['ema']
    assert d['pool_size'] == 13 and d['weights'] == 'ema' and d['score'] == 'margin' and d['num_clusters'] == 3
    assert len(d['clusters']) == 3 and sum(c['size'] for c in d['clusters']) == 13
    assert all(len(c['selected']) == min(2, c['size']) for c in d['clusters'])
    assert sorted(r['image'] for r in d['ranking']) == [f'img_{i:02d}.jpg' for i in range(13)]
    m = [r['margin'] for r in d['ranking']]
    assert m == sorted(m, reverse=True) and all(np.isfinite([r['entropy'], r['least_confidence']]).all()
                                                for r in d['ranking'])
    for c in d['clusters']:                                            # the selected are the cluster's top margins
        members = [r for r in d['ranking'] if r['cluster'] == c['cluster']]
        assert [r['index'] for r in members[:2]] == [r['index'] for r in c['selected']]
    # the two weight sets are different models: different scores
    assert [r['entropy'] for r in d['ranking']] != [r['entropy'] for r in docs['student']['ranking']]
