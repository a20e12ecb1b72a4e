"""fp64 numpy restatement of the active-learning rules of csrc/active.hip / ssseg/active.py, the checker of the
test_active_* files.

Reference: get_active_learning_partition.py -- entropy :94-95 (softmax, -(p log p).sum(1).mean()), pooled features
:96-99, KMeans(n_clusters=10, tol=1e-6, max_iter=300) :118, per-cluster stable sort(reverse=True) and the first five
:128-134.  The scores are written in the stable form log Z - sum p (x - m) (a saturated pixel scores 0, where :95
gives NaN); least confidence and margin are the two companions of the entropy.  k-means: k-means++ from given
uniforms with the scan rule of include/ssseg.h, lowest-index ties, keep-on-empty, sklearn's tolerance rule with the
population variance, and a last assignment against the returned centroids.
"""
import numpy as np


def scores(x, dtype=np.float64):
    """x [B,C,...] -> [B,3] (entropy, least confidence, margin), every operation in `dtype`, the means in fp64"""
    x = np.asarray(x).astype(dtype)
    B, C = x.shape[:2]
    x = x.reshape(B, C, -1)
    m = x.max(1, keepdims=True)
    d = x - m
    e = np.exp(d)
    z = e.sum(1, keepdims=True)
    h = (np.log(z) - (e * d).sum(1, keepdims=True) / z)[:, 0]
    top = np.sort(x, axis=1)[:, ::-1][:, :2]                         # the two largest logits (a tie gives equal ones)
    inv = (dtype(1) / z)[:, 0]
    p2 = np.exp(top[:, 1] - top[:, 0]) * inv
    lc = dtype(1) - inv
    mg = dtype(1) - (inv - p2)
    return np.stack([h.astype(np.float64).mean(1), lc.astype(np.float64).mean(1), mg.astype(np.float64).mean(1)], 1)


def reference_entropy(x):
    """the reference's own expression (:94-95) in fp64: NaN once a probability underflows"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(-(p * np.log(p)).sum(1).mean())


def _sqdist(X, c):
    """|x_i - c|^2 for every row, summed in the order include/ssseg.h states for the device: 64 lanes, lane l adds the
    squares of d = l, l + 64, ... in that order, then the lanes are summed by the xor butterfly 32, 16, ..., 1 (so
    data on which every square is exact gives the same bits whatever the order, and any other data the same bits as
    the device)."""
    t = X - c
    t = t * t
    n, d = t.shape
    chunks = -(-d // 64)
    lanes = np.zeros((n, chunks * 64))
    lanes[:, :d] = t
    lanes = lanes.reshape(n, chunks, 64)
    acc = np.zeros((n, 64))
    for j in range(chunks):
        acc = acc + lanes[:, j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


def _ordered_sum(v, threads=1024):
    """sum in the device's order: `threads` contiguous slices of ceil(n / threads) elements, each summed in index order,
    the slice sums added in slice order"""
    v = np.asarray(v, np.float64)
    per = -(-len(v) // threads)
    total = 0.0
    for lo in range(0, len(v), per):
        s = 0.0
        for a in v[lo:lo + per]:
            s += float(a)
        total += s
    return total


def seed(X, u, k):
    """k-means++ from the uniforms u[k] -> (seed_idx [k], smallest relative distance of a threshold from a scan
    boundary).  First centre min(floor(u0 N), N - 1); centre j the first i whose inclusive cumulative sum of d2 exceeds
    u_j * sum(d2) (N - 1 if none does)."""
    X = np.asarray(X, np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    N = X.shape[0]
    idx = [min(int(np.floor(u[0] * N)), N - 1)]
    d2 = _sqdist(X, X[idx[0]])
    gap = np.inf
    for j in range(1, k):
        cum = np.cumsum(d2)
        thr = u[j] * cum[-1]
        hit = np.nonzero(cum > thr)[0]
        idx.append(int(hit[0]) if hit.size else N - 1)
        if cum[-1] > 0:
            gap = min(gap, float(np.abs(cum - thr).min() / cum[-1]))
        d2 = np.minimum(d2, _sqdist(X, X[idx[-1]]))
    return np.asarray(idx, np.int32), gap


def assign(X, cent):
    """-> (labels, squared distance to the own centroid, smallest relative gap between best and second best)"""
    d = np.stack([_sqdist(X, c) for c in cent], 1)
    lab = d.argmin(1)                                                # the first minimum: the lowest index on a tie
    best = d[np.arange(len(X)), lab]
    gap = np.inf
    if d.shape[1] > 1:
        second = np.partition(d, 1, axis=1)[:, 1]
        gap = float(((second - best) / np.maximum(second, np.finfo(np.float64).tiny)).min())
    return lab.astype(np.int32), best, gap


def lloyd(X, init, tol=1e-6, max_iter=300):
    """-> dict(centroids, labels, inertia, n_iter, gap).  Stops once sum |c_new - c_old|^2 <= tol * mean_d Var(X[:,d])."""
    X = np.asarray(X, np.float32).astype(np.float64)
    cent = np.array(init, np.float64, copy=True)
    thr = tol * X.var(0).mean()
    gap, n_iter = np.inf, 0
    for _ in range(max_iter):
        lab, _, g = assign(X, cent)
        gap = min(gap, g)
        new = cent.copy()
        for k in range(len(cent)):
            pts = X[lab == k]
            if len(pts):                                             # an empty cluster keeps its centroid
                new[k] = pts.sum(0) / len(pts)
        shift = float(((new - cent) ** 2).sum())
        cent = new
        n_iter += 1
        if shift <= thr:
            break
    lab, best, g = assign(X, cent)
    return dict(centroids=cent, labels=lab, inertia=_ordered_sum(best), n_iter=n_iter, gap=min(gap, g))


def kmeans(X, k, u=None, init=None, tol=1e-6, max_iter=300):
    X = np.asarray(X, np.float32)
    seeds, sgap = None, np.inf
    if u is not None:
        seeds, sgap = seed(X, u, k)
        init = X[seeds].astype(np.float64)
    out = lloyd(X, init, tol, max_iter)
    out.update(seed_idx=seeds, seed_gap=sgap)
    return out


def rank(score):
    """indices by descending score, ties to the lower index"""
    return sorted(range(len(score)), key=lambda i: (-float(score[i]), i))


def select(score, labels, per_cluster, k):
    """per cluster the per_cluster highest scores, ties to the lower pool index (:128-134)"""
    out = []
    for c in range(k):
        members = [i for i in range(len(labels)) if int(labels[i]) == c]
        members.sort(key=lambda i: float(score[i]), reverse=True)    # stable, as the reference's :130
        out.append(members[:per_cluster])
    return out
