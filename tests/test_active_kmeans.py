"""GPU: ops.kmeans (csrc/active.hip) against the fp64 oracle of active_ref.py.  Every dataset comes from a seeded numpy
generator (the generators of test_active_host.py, where the oracle itself is checked against scipy).

Integer blobs: every distance and sum is exact in fp64, so seeds, labels, n_iter and inertia must equal the oracle's and
the centroids agree to rtol 1e-12 (the division).  Overlapping blobs: the test first asserts that no decision of the
oracle is closer than 1e-9 (relative) to a tie -- the device differs from the oracle by the fp64 summation order only,
some 1e-13 -- so no point is excused: equal seeds, labels and n_iter, centroids and inertia within rtol 1e-9."""
import numpy as np
import pytest
import torch

import active_ref as R
from test_active_host import KMEANS_CASES, dataset

pytestmark = pytest.mark.gpu


def run(X, k, dev, **kw):
    from ssseg import ops
    r = ops.kmeans(torch.from_numpy(X).to(dev), k, **kw)
    return dict(centroids=r.centroids.cpu().numpy(), labels=r.labels.cpu().numpy(), inertia=float(r.inertia),
                n_iter=int(r.n_iter), seed_idx=None if r.seed_idx is None else r.seed_idx.cpu().numpy())


def compare(got, o, rtol, exact_inertia=False, atol=0.0):
    print('n_iter', got['n_iter'], o['n_iter'], 'inertia', got['inertia'], o['inertia'], 'centroid error',
          np.abs(got['centroids'] - o['centroids']).max())
    if o.get('seed_idx') is not None:
        assert np.array_equal(got['seed_idx'], o['seed_idx'])
    assert np.array_equal(got['labels'], o['labels'])
    assert got['n_iter'] == o['n_iter']
    if exact_inertia:
        assert got['inertia'] == o['inertia']
    else:
        np.testing.assert_allclose(got['inertia'], o['inertia'], rtol=rtol, atol=0)
    np.testing.assert_allclose(got['centroids'], o['centroids'], rtol=rtol, atol=atol)


@pytest.mark.parametrize('kind,s', KMEANS_CASES)
def test_kmeans_matches_oracle(hip_device, kind, s):
    X, u, K = dataset(kind, s)
    o = R.kmeans(X, K, u=u)
    print(kind, s, 'oracle gaps', o['gap'], o['seed_gap'])
    assert o['gap'] >= 1e-9 and o['seed_gap'] >= 1e-9
    got = run(X, K, hip_device, u=torch.from_numpy(u))
    assert got['labels'].dtype == np.int32 and got['centroids'].dtype == np.float64
    if kind == 'int':
        compare(got, o, 1e-12, exact_inertia=True)
    else:
        compare(got, o, 1e-9)


def test_wide_features(hip_device):
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((10, 2048))[rng.integers(0, 10, 64)] * 0.2 + rng.standard_normal((64, 2048))).astype(
        np.float32)
    u = rng.random(10).astype(np.float32)
    o = R.kmeans(X, 10, u=u)
    assert o['gap'] >= 1e-9 and o['seed_gap'] >= 1e-9
    compare(run(X, 10, hip_device, u=u), o, 1e-9)


# edge cases on 41 standard-normal points: a centroid coordinate can cancel towards 0, so next to rtol the bound is the
# rounding of a 41-term fp64 sum, 41 * 2^-53 * sum |x| < 41 * 1.2e-16 * 41 * 5 < 1e-12 (absolute)
EDGE = dict(rtol=1e-12, atol=1e-12)


def _small(seed=3, n=41, d=5):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def test_single_cluster(hip_device):
    X = _small()
    got = run(X, 1, hip_device, u=[0.37])
    o = R.kmeans(X, 1, u=[0.37])
    compare(got, o, **EDGE)
    assert (got['labels'] == 0).all() and got['seed_idx'].tolist() == [int(0.37 * 41)]
    np.testing.assert_allclose(got['centroids'][0], X.astype(np.float64).mean(0), **EDGE)


def test_empty_cluster_keeps_its_centroid(hip_device):
    X = _small()
    init = np.concatenate([X[:2].astype(np.float64), np.full((1, 5), 1e3)])
    got = run(X, 3, hip_device, init=torch.from_numpy(init))
    compare(got, R.kmeans(X, 3, init=init), **EDGE)
    assert got['seed_idx'] is None and (got['labels'] != 2).all()
    assert np.array_equal(got['centroids'][2], init[2])


def test_identical_centroids_lower_index_wins(hip_device):
    X = _small()
    init = np.stack([X[7], X[7], X[20]]).astype(np.float64)
    got = run(X, 3, hip_device, init=init, max_iter=1)
    o = R.kmeans(X, 3, init=init, max_iter=1)
    # one iteration: cluster 1 received nothing and still sits on X[7]
    assert np.array_equal(got['centroids'][1], init[1]) and got['n_iter'] == 1
    compare(got, o, **EDGE)
    first = R.assign(X.astype(np.float64), init)[0]
    assert (first != 1).all()


def test_max_iter_and_early_stop(hip_device):
    X, u, K = dataset('o515', 0)
    o = R.kmeans(X, K, u=u)
    assert 1 < o['n_iter'] < 300
    assert run(X, K, hip_device, u=u, max_iter=1)['n_iter'] == 1
    assert run(X, K, hip_device, u=u, max_iter=300)['n_iter'] == o['n_iter']
    part = R.kmeans(X, K, u=u, max_iter=3)
    compare(run(X, K, hip_device, u=u, max_iter=3), part, 1e-9)


def test_two_runs_are_bitwise_identical(hip_device):
    X, u, K = dataset('o1031', 1)
    a, b = run(X, K, hip_device, u=u), run(X, K, hip_device, u=u)
    assert a['centroids'].tobytes() == b['centroids'].tobytes() and a['inertia'] == b['inertia']
    assert np.array_equal(a['labels'], b['labels']) and a['n_iter'] == b['n_iter']


def test_refusals(hip_device):
    from ssseg import native as N
    from ssseg import ops
    X = torch.from_numpy(_small()).to(hip_device)
    for k in (0, 65, 42):
        with pytest.raises(ValueError):
            ops.kmeans(X, k, u=[0.5] * max(k, 1))
        assert N.lib().ssseg_kmeans_workspace_bytes(41, 5, k) == 0
    with pytest.raises(ValueError, match='exactly one'):
        ops.kmeans(X, 2)
    with pytest.raises(ValueError, match='exactly one'):
        ops.kmeans(X, 2, u=[0.1, 0.2], init=X[:2])
    with pytest.raises((RuntimeError, ValueError), match='HIP device tensor'):
        ops.kmeans(X.cpu(), 2, u=[0.1, 0.2])
    with pytest.raises(ValueError):
        ops.kmeans(X, 2, u=[0.1, 1.0])
    with pytest.raises(ValueError):
        ops.kmeans(X, 2, init=X[:3])
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=hip_device)
    assert N.lib().ssseg_kmeans_fit(X.data_ptr(), 41, 5, 65, 1e-6, 10, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(),
                                    ws.data_ptr(), ws.data_ptr(), 1 << 16, None) == -1
