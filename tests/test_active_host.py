"""No GPU: the active-learning oracle (tests/active_ref.py) against scipy and the golden entropy, the selection and
ranking rules, the entry point's argument handling and JSON schema with a stub scorer, and the ABI bookkeeping."""
import json
import os

import numpy as np
import pytest
import torch

import active_ref as R
from conftest import PKG, golden


# ---- datasets of tests/test_active_kmeans.py (kept identical there) ----
def integer_blobs(s):
    rng = np.random.default_rng(100 + s)
    u = rng.random(3)
    cent = np.zeros((3, 8))
    cent[1] = 40
    cent[2] = np.where(np.arange(8) % 2 == 0, -40, 40)
    lab = np.arange(97) % 3
    X = cent[lab] + rng.integers(-3, 4, size=(97, 8))
    return X.astype(np.float32), u.astype(np.float32)


def overlapping_blobs(N, D, K, spread, s):
    rng = np.random.default_rng(s)
    cent = rng.standard_normal((K, D)) * spread
    X = cent[rng.integers(0, K, N)] + rng.standard_normal((N, D))
    return X.astype(np.float32), np.random.default_rng(1000 + s).random(K).astype(np.float32)


KMEANS_CASES = ([('int', s) for s in range(3)] + [('o515', s) for s in range(4)] + [('o1031', s) for s in range(2)])


def dataset(kind, s):
    if kind == 'int':
        return integer_blobs(s) + (3,)
    if kind == 'o515':
        return overlapping_blobs(515, 16, 5, 1.0, s) + (5,)
    return overlapping_blobs(1031, 130, 10, 0.35, s) + (10,)


@pytest.mark.parametrize('kind,s', KMEANS_CASES)
def test_oracle_kmeans_matches_scipy(kind, s):
    from scipy.cluster.vq import kmeans2
    X, u, K = dataset(kind, s)
    o = R.kmeans(X, K, u=u)
    init = X[o['seed_idx']].astype(np.float64)
    cent, lab = kmeans2(X.astype(np.float64), init, iter=o['n_iter'], minit='matrix')
    print(kind, s, 'n_iter', o['n_iter'], 'gap', o['gap'], 'seed gap', o['seed_gap'])
    assert np.array_equal(lab, o['labels'])
    np.testing.assert_allclose(cent, o['centroids'], rtol=1e-9, atol=0)
    assert o['gap'] >= 1e-9 and o['seed_gap'] >= 1e-9
    if kind == 'int':
        assert o['n_iter'] == 2
    else:
        assert 5 <= o['n_iter'] <= 15


def test_oracle_rules_on_hand_made_data():
    X = np.array([[0.], [1.], [10.], [11.]], np.float32)
    # two identical initial centroids: the lower index takes the points; a far centroid stays empty and unchanged
    init = np.array([[0.5], [0.5], [1000.]])
    assert R.assign(X.astype(np.float64), init)[0].tolist() == [0, 0, 0, 0]
    o = R.lloyd(X, init, max_iter=1)
    assert o['centroids'][:, 0].tolist() == [5.5, 0.5, 1000.] and o['labels'].tolist() == [1, 1, 0, 0]
    # seeding: first = floor(u0 N); then the first index whose inclusive cumulative sum exceeds u * total
    idx, _ = R.seed(X, [0.0, 0.5], 2)                       # d2 = [0, 1, 100, 121], total 222, thr 111 -> index 3
    assert idx.tolist() == [0, 3]
    idx, _ = R.seed(X, [0.99, 0.0], 2)                      # first = 3; d2 = [121, 100, 1, 0], thr 0 -> index 0
    assert idx.tolist() == [3, 0]
    # the tolerance rule: one iteration moves the centroids, the second does not
    o = R.lloyd(X, np.array([[0.], [11.]]))
    assert o['n_iter'] == 2 and o['centroids'][:, 0].tolist() == [0.5, 10.5] and o['inertia'] == 1.0
    assert R.lloyd(X, np.array([[0.], [11.]]), max_iter=1)['n_iter'] == 1


def test_oracle_entropy_matches_golden():
    g = golden('active_entropy.npz')
    n = 0
    while f'logits{n}' in g:
        x, ref = g[f'logits{n}'], g[f'entropy{n}']
        got = R.scores(x)[:, 0]
        print(x.shape, np.abs(got - ref).max())
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose([R.reference_entropy(x[b:b + 1]) for b in range(len(x))], ref, rtol=1e-12)
        n += 1
    assert n >= 4


def test_oracle_scores_designed_cases():
    C = 5
    s = R.scores(np.zeros((1, C, 2, 3)))
    np.testing.assert_allclose(s[0], [np.log(C), 1 - 1 / C, 1.0], rtol=1e-15)
    x = np.zeros((1, C, 2, 2))
    x[:, 1] = 200.0
    assert R.scores(x, np.float32)[0].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(R.reference_entropy(x.astype(np.float32).astype(np.float64) * 4))    # the reference's form: NaN
    x[:, 3] = 200.0
    s = R.scores(x)
    np.testing.assert_allclose(s[0], [np.log(2), 0.5, 1.0], rtol=1e-12)


def test_fp32_evaluation_error_is_small():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 19, 5, 7)) * 3).astype(np.float32)
    err = np.abs(R.scores(x, np.float32) - R.scores(x)) / np.abs(R.scores(x))
    print('fp32 relative error', err.max())
    assert err.max() < 1e-6


def test_select_and_rank_ties():
    from ssseg import active
    scores = torch.tensor([[0.5, 0, 0], [0.9, 0, 1], [0.5, 0, 2], [0.9, 0, 3], [0.1, 0, 4], [0.5, 0, 5]])
    labels = torch.tensor([0, 0, 0, 1, 1, 0], dtype=torch.int32)
    assert active.rank(scores, 0) == [1, 3, 0, 2, 5, 4]
    assert active.rank(scores, 'margin') == [5, 4, 3, 2, 1, 0]
    assert active.select(scores, labels, per_cluster=2, column=0) == [[1, 0], [3, 4]]
    assert active.select(scores, labels, per_cluster=5, column=0, num_clusters=3) == [[1, 0, 2, 5], [3, 4], []]
    assert active.select(scores, labels, 2, 0) == R.select(scores[:, 0].tolist(), labels.tolist(), 2, 2)
    assert active.rank(scores, 0) == R.rank(scores[:, 0].tolist())
    with pytest.raises(ValueError):
        active.rank(scores, 'variance')
    with pytest.raises(ValueError):
        active.select(scores, labels[:3])


def _cfg_file(tmp_path, body=''):
    p = tmp_path / 'al_cfg.py'
    p.write_text("common = dict(image_size=64)\nmodel = dict(model_fn=None)\n" + body)
    return str(p)


def _stub(cfg, args, s):
    from ssseg import active
    n = 7
    scores = torch.tensor([[i % 3, (i * 5) % 7, i] for i in range(n)], dtype=torch.float32) / 10
    labels = torch.tensor([i % s['num_clusters'] for i in range(n)], dtype=torch.int32)
    res = dict(scores=scores, labels=labels, n_iter=torch.tensor(4, dtype=torch.int32),
               inertia=torch.tensor(1.5, dtype=torch.float64),
               clusters=active.select(scores, labels, s['per_cluster'], s['score'], s['num_clusters']),
               ranking=active.rank(scores, s['score']))
    return [f'/pool/img{i}.jpg' for i in range(n)], res


def test_cli_arguments_and_json_schema(tmp_path):
    import get_active_learning_partition as cli
    out = tmp_path / 'part.json'
    cfg = _cfg_file(tmp_path, "active_learning = dict(num_clusters=3, per_cluster=1, score='margin')\n")
    doc = cli.main([cfg, '--checkpoint', 'ck.pth', '--images', 'a', 'b', '--per-cluster', '2', '--out', str(out)],
                   scorer=_stub)
    assert json.loads(out.read_text()) == doc
    # command line > cfg['active_learning'] > defaults
    assert (doc['num_clusters'], doc['per_cluster'], doc['score'], doc['weights'], doc['seed']) == (3, 2, 'margin',
                                                                                                     'ema', 0)
    assert doc['pool_size'] == 7 and doc['n_iter'] == 4 and doc['inertia'] == 1.5
    assert [c['cluster'] for c in doc['clusters']] == [0, 1, 2] and [c['size'] for c in doc['clusters']] == [3, 2, 2]
    for c in doc['clusters']:
        assert 1 <= len(c['selected']) <= 2
        for r in c['selected']:
            assert set(r) == {'image', 'index', 'entropy', 'least_confidence', 'margin'}
            assert r['image'] == f"img{r['index']}.jpg" and r['index'] % 3 == c['cluster']
    assert [r['index'] for r in doc['ranking']] == [6, 5, 4, 3, 2, 1, 0]              # by margin, descending
    assert set(doc['ranking'][0]) == {'image', 'index', 'cluster', 'entropy', 'least_confidence', 'margin'}
    assert doc['clusters'][0]['selected'][0]['index'] == 6

    # without the key: the defaults
    a = cli.parse_args([_cfg_file(tmp_path), '--checkpoint', 'c', '--images', 'd', '--out', 'o'])
    assert cli.settings(a, {}) == cli.DEFAULTS
    assert cli.settings(a, {'active_learning': {'seed': 3}})['seed'] == 3
    with pytest.raises(ValueError):
        cli.settings(a, {'active_learning': {'clusters': 3}})
    with pytest.raises(ValueError):
        cli.settings(cli.parse_args(['c.py', '--checkpoint', 'c', '--images', 'd', '--out', 'o', '--num-clusters',
                                     '65']), {})
    for bad in (['c.py', '--images', 'd', '--out', 'o'], ['c.py', '--checkpoint', 'c', '--out', 'o'],
                ['c.py', '--checkpoint', 'c', '--images', 'd'],
                ['c.py', '--checkpoint', 'c', '--images', 'd', '--out', 'o', '--score', 'variance'],
                ['c.py', '--checkpoint', 'c', '--images', 'd', '--out', 'o', '--weights', 'teacher']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_validation_transforms_default():
    import get_active_learning_partition as cli
    aug = cli.validation_transforms({'common': {'image_size': 32}})
    img = aug(image=np.full((10, 20, 3), 255, np.uint8))['image']
    assert img.shape == (32, 32, 3) and img.dtype == np.float32 and img.max() == 1.0
    marker = object()
    assert cli.validation_transforms({'common': {}, 'val': {'augmentations': marker}}) is marker


def test_header_and_sigs_list_the_new_symbols():
    from ssseg import native
    new = {'ssseg_uncertainty_workspace_bytes', 'ssseg_uncertainty_scores', 'ssseg_kmeans_workspace_bytes',
           'ssseg_kmeans_seed', 'ssseg_kmeans_fit'}
    assert new <= set(native.header_symbols()) and new <= set(native.SIGS)
    lib = native.lib()
    # refused on the host before any launch
    assert lib.ssseg_uncertainty_scores(None, 1, 2, 4, None, None, 0, None) == -1
    assert lib.ssseg_uncertainty_workspace_bytes(1, 1, 4) == 0 and lib.ssseg_uncertainty_workspace_bytes(1, 65, 4) == 0
    assert lib.ssseg_uncertainty_workspace_bytes(3, 2, 4) == 3 * 3 * 8
    assert lib.ssseg_kmeans_workspace_bytes(10, 4, 0) == 0 and lib.ssseg_kmeans_workspace_bytes(10, 4, 65) == 0
    assert lib.ssseg_kmeans_workspace_bytes(3, 4, 4) == 0 and lib.ssseg_kmeans_workspace_bytes(10, 4, 3) > 0
    assert lib.ssseg_kmeans_seed(None, 10, 4, 3, None, None, None, None, 0, None) == -1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from ssseg import ops
    with pytest.raises((RuntimeError, ValueError), match='HIP device tensor'):
        ops.uncertainty_scores(torch.zeros(1, 2, 4, 4))
    with pytest.raises((RuntimeError, ValueError), match='HIP device tensor'):
        ops.kmeans(torch.zeros(8, 2), 2, u=[0.1, 0.2])
    for c in (1, 65):
        with pytest.raises(ValueError, match='channels'):
            ops.uncertainty_scores(torch.zeros(1, c, 2, 2))


def test_sources_name_the_deviation():
    src = open(os.path.join(PKG, 'csrc', 'active.hip')).read()
    assert 'DEVIATION' in src and 'NaN' in src
