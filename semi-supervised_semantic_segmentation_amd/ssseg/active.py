"""Active-learning pool selection: score an unlabelled pool with a trained model, cluster the images by their
features and pick the most uncertain images of every cluster (the reference's get_active_learning_partition.py, with
get_least_confident_images.py's ranking next to it; no database, object store, cv2 or sklearn).

    scores, features = score_pool(model, loader)          # device tensors, one row per pool item in loader order
    result = partition(model, loader, num_clusters=10)    # scoring + k-means++ + Lloyd + selection

The scores are ops.uncertainty_scores (entropy, least confidence, margin; csrc/active.hip), the clustering is
ops.kmeans.  Which `feature_source` a model family needs:

  * models that return real features (HigherHRNet, the multi-scale attention model): 'model' -- features[-1] as the
    reference takes it (:96-99);
  * models wrapped by models.adapters.ListOutput (SimpleUNet, UNet, DeepLabV3, HarDNet) return `[y], [y]`, so
    'model' clusters on the pooled logits (C numbers per image).  Name a submodule instead: 'encoder' for models.unet
    (its last endpoint, 2048 wide for ResNet-50), 'backbone' for DeepLabV3; any name of model.named_modules() works,
    with or without the wrapper's 'model.' prefix.  The module's forward output (the last element of a list or tuple)
    is captured with a forward hook.  SimpleUNet's encoder is a ModuleList whose stages are never called as modules:
    name the DownBlock of a stage, e.g. 'encoder.3.1'.
"""
import torch

from . import nn as snn
from . import ops

SCORE_COLUMNS = {'entropy': 0, 'least_confidence': 1, 'margin': 2}


def _column(column):
    if isinstance(column, str):
        if column not in SCORE_COLUMNS:
            raise ValueError(f'score column must be one of {sorted(SCORE_COLUMNS)}, got {column!r}')
        return SCORE_COLUMNS[column]
    column = int(column)
    if not 0 <= column <= 2:
        raise ValueError(f'score column must be 0, 1 or 2, got {column}')
    return column


def _images(batch):
    if isinstance(batch, dict):
        return batch['image']
    if isinstance(batch, (list, tuple)):
        return batch[0]
    return batch


def _find_module(model, name):
    mods = dict(model.named_modules())
    for cand in (name, 'model.' + name):
        if cand in mods:
            return mods[cand]
    raise ValueError(f'score_pool: feature_source {name!r} is neither "model" nor a submodule of {type(model).__name__}')


def pooled_features(f, channels=None):
    """[n,C,h,w] feature map (an NHWC activation of the model, or any NCHW float tensor) -> [n,channels] fp32 rows of
    its global average (snn.global_avgpool); `channels` cuts padded channels off (default: all of them)."""
    if f.dim() != 4:
        raise ValueError(f'score_pool: a [n,C,h,w] feature map is needed, got {tuple(f.shape)}')
    n, c = f.shape[:2]
    a = f if snn._is_act(f) and c % snn.vec() == 0 else snn.to_act(f.detach())
    y = snn.global_avgpool(a)
    return y.reshape(n, y.shape[1])[:, :(c if channels is None else channels)].float()


def score_pool(model, loader, feature_source='model', device=None):
    """-> (scores [N,3], features [N,D]) fp32 device tensors, one row per pool item in loader order.  The model runs
    in eval mode under no_grad (its mode is restored); logits are logit_resolutions[-1] at the model's own output
    resolution (:94); features are features[-1], or the output of the submodule named by `feature_source`, averaged
    over each image (:96-99)."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'ssseg: score_pool needs a HIP device tensor path (no CPU fallback), got device {device}')
    captured, handle, channels = [], None, None
    if feature_source != 'model':
        mod = _find_module(model, feature_source)
        depths = getattr(mod, 'endpoint_depths', None)
        channels = int(depths[-1]) if depths else None
        handle = mod.register_forward_hook(lambda m, i, o: captured.append(o[-1] if isinstance(o, (list, tuple)) else o))
    was_training = model.training
    model.eval()
    scores, feats = [], []
    try:
        with torch.no_grad():
            for batch in loader:
                x = _images(batch).to(device, non_blocking=True)
                del captured[:]
                features, logit_resolutions = model(x)
                scores.append(ops.uncertainty_scores(logit_resolutions[-1]))
                if handle is None:
                    feats.append(pooled_features(features[-1]))
                else:
                    if not captured:
                        raise RuntimeError(f'score_pool: submodule {feature_source!r} did not run in the forward pass')
                    feats.append(pooled_features(captured[-1], channels))
    finally:
        if handle is not None:
            handle.remove()
        model.train(was_training)
    if not scores:
        raise ValueError('score_pool: the pool is empty')
    return torch.cat(scores), torch.cat(feats)


def rank(scores, column=0):
    """Pool indices sorted by one score, most uncertain first; ties go to the lower index (the useful half of
    get_least_confident_images.py)."""
    s = torch.as_tensor(scores).detach().cpu()
    col = s[:, _column(column)] if s.dim() == 2 else s
    return torch.sort(col, descending=True, stable=True).indices.tolist()


def select(scores, labels, per_cluster=5, column=0, num_clusters=None):
    """Per cluster, the `per_cluster` highest-scoring pool indices, ties to the lower pool index (the reference's
    stable sort(reverse=True), :130).  -> a list of num_clusters (default: max label + 1) lists of pool indices."""
    labels = torch.as_tensor(labels).detach().cpu().long()
    s = torch.as_tensor(scores).detach().cpu()
    if s.shape[0] != labels.shape[0]:
        raise ValueError(f'select: {s.shape[0]} score rows for {labels.shape[0]} labels')
    if per_cluster < 0:
        raise ValueError(f'select: per_cluster = {per_cluster}')
    k = int(labels.max()) + 1 if num_clusters is None else int(num_clusters)
    order = rank(s, column)
    out = [[] for _ in range(k)]
    lab = labels.tolist()
    for i in order:
        if len(out[lab[i]]) < per_cluster:
            out[lab[i]].append(i)
    return out


def partition(model, loader, num_clusters=10, per_cluster=5, seed=0, n_init=1, column=0, feature_source='model',
              tol=1e-6, max_iter=300, device=None):
    """The whole pipeline: score the pool, seed k-means++ from a torch.Generator seeded with `seed`, fit, select.
    With n_init > 1 every fit is enqueued first and the one with the lowest inertia wins (the first on a tie).
    -> dict(scores, features, labels, centroids, inertia, n_iter, seed_idx, clusters, ranking)."""
    if n_init < 1:
        raise ValueError(f'partition: n_init = {n_init}')
    scores, features = score_pool(model, loader, feature_source, device)
    g = torch.Generator().manual_seed(int(seed))
    fits = [ops.kmeans(features, num_clusters, u=torch.rand(num_clusters, generator=g), tol=tol, max_iter=max_iter)
            for _ in range(n_init)]
    inertias = torch.stack([f.inertia for f in fits]).cpu().tolist()
    best = fits[min(range(n_init), key=lambda i: (inertias[i], i))]
    return dict(scores=scores, features=features, labels=best.labels, centroids=best.centroids, inertia=best.inertia,
                n_iter=best.n_iter, seed_idx=best.seed_idx,
                clusters=select(scores, best.labels, per_cluster, column, num_clusters), ranking=rank(scores, column))
