"""Pick the next images to label -- the reference's get_active_learning_partition.py (entropy :94-95, pooled features
:96-99, KMeans(10, tol=1e-6, max_iter=300) :118, the five highest-entropy images of every cluster :128-134) with
get_least_confident_images.py's ranking, on the device and without its database, object store, cv2 and sklearn:

    get_active_learning_partition.py CONFIG --checkpoint PATH --images DIR [DIR...]
        [--weights ema|student] [--num-clusters 10] [--per-cluster 5]
        [--score entropy|least_confidence|margin] [--seed 0] [--features SOURCE] [--batch-size 8] --out FILE.json

The model is built from the config as distributed_trainer does, the checkpoint read by its dict keys (default
ema_state_dict, the teacher), the pool read through UnsupervisedImagesDataset with the validation-time transforms
(val['augmentations'] of the config, else LongestMaxSize + PadIfNeeded to common['image_size'] + ToFloat, the
reference's :21-24).  An optional cfg['active_learning'] dict (num_clusters, per_cluster, score, seed, weights,
feature_source, batch_size, n_init) supplies defaults; the command line wins.  FILE.json:

    {"config", "checkpoint", "weights", "score", "seed", "num_clusters", "per_cluster", "feature_source", "pool_size",
     "n_iter", "inertia",
     "clusters": [{"cluster": k, "size": n_k, "selected": [{"image", "index", "entropy", "least_confidence", "margin"}]}],
     "ranking": [{"image", "index", "cluster", "entropy", "least_confidence", "margin"}]}      # most uncertain first
"""
import argparse
import json
import os
import sys

DEFAULTS = dict(num_clusters=10, per_cluster=5, score='entropy', seed=0, weights='ema', feature_source='model',
                batch_size=8, n_init=1)
SCORES = ('entropy', 'least_confidence', 'margin')
WEIGHT_KEYS = {'ema': 'ema_state_dict', 'student': 'state_dict'}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Cluster an unlabelled pool and select the most uncertain images of '
                                            'every cluster.')
    p.add_argument('config')
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--images', nargs='+', required=True, metavar='DIR')
    p.add_argument('--weights', choices=sorted(WEIGHT_KEYS))
    p.add_argument('--num-clusters', type=int)
    p.add_argument('--per-cluster', type=int)
    p.add_argument('--score', choices=SCORES)
    p.add_argument('--seed', type=int)
    p.add_argument('--features', dest='feature_source', metavar='SOURCE',
                   help="'model' (features[-1]) or a submodule name such as 'encoder' (see ssseg/active.py)")
    p.add_argument('--batch-size', type=int)
    p.add_argument('--out', required=True, metavar='FILE.json')
    return p.parse_args(argv)


def settings(args, cfg):
    """command line > cfg['active_learning'] > DEFAULTS, validated"""
    s = dict(DEFAULTS)
    extra = set(cfg.get('active_learning') or {}) - set(DEFAULTS)
    if extra:
        raise ValueError(f"cfg['active_learning']: unknown keys {sorted(extra)}")
    s.update(cfg.get('active_learning') or {})
    for k in DEFAULTS:
        v = getattr(args, k, None)
        if v is not None:
            s[k] = v
    if s['score'] not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {s['score']!r}")
    if s['weights'] not in WEIGHT_KEYS:
        raise ValueError(f"weights must be 'ema' or 'student', got {s['weights']!r}")
    if not 1 <= s['num_clusters'] <= 64:
        raise ValueError(f"num_clusters = {s['num_clusters']} (1 .. 64)")
    if s['per_cluster'] < 1 or s['batch_size'] < 1 or s['n_init'] < 1:
        raise ValueError(f"per_cluster, batch_size and n_init must be positive, got {s}")
    return s


def document(names, scores, labels, clusters, ranking, meta):
    """The JSON document from plain lists: names [N], scores [N][3], labels [N], clusters [K][<= per_cluster],
    ranking [N]."""
    def row(i, with_cluster):
        r = {'image': names[i], 'index': int(i)}
        if with_cluster:
            r['cluster'] = int(labels[i])
        r.update({k: float(scores[i][j]) for j, k in enumerate(SCORES)})
        return r
    doc = dict(meta)
    doc['pool_size'] = len(names)
    doc['clusters'] = [{'cluster': k, 'size': sum(1 for l in labels if l == k), 'selected': [row(i, False) for i in sel]}
                       for k, sel in enumerate(clusters)]
    doc['ranking'] = [row(i, True) for i in ranking]
    return doc


def validation_transforms(cfg):
    from data import transforms as T
    aug = (cfg.get('val') or {}).get('augmentations')
    if aug is not None:
        return aug
    size = int(cfg['common']['image_size'])
    return T.Compose([T.LongestMaxSize(max_size=size), T.PadIfNeeded(min_height=size, min_width=size), T.ToFloat()])


def score_and_partition(cfg, args, s):
    """-> (names, result of ssseg.active.partition) on cuda:0"""
    import torch

    from data.unsupervised_dataset import UnsupervisedImagesDataset
    from ssseg import active
    from ssseg import nn as snn

    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    snn.set_compute_dtype({'fp32': torch.float32, 'fp16': torch.float16}.get(cfg['common'].get('compute_dtype'),
                                                                             torch.bfloat16))
    model = cfg['model']['model_fn']().to(device)
    ck = torch.load(args.checkpoint, map_location='cpu')
    key = WEIGHT_KEYS[s['weights']]
    if key not in ck:
        raise KeyError(f'{args.checkpoint}: no {key!r} (keys: {sorted(ck)})')
    model.load_state_dict(ck[key], strict=False)
    pool = UnsupervisedImagesDataset(args.images, validation_transforms(cfg))
    pool.filenames.sort()
    if len(pool) < s['num_clusters']:
        raise ValueError(f"{len(pool)} images under {args.images} for {s['num_clusters']} clusters")
    loader = torch.utils.data.DataLoader(pool, batch_size=s['batch_size'], shuffle=False,
                                         num_workers=int((cfg.get('val') or {}).get('num_dataloader_workers', 0)))
    res = active.partition(model, loader, num_clusters=s['num_clusters'], per_cluster=s['per_cluster'],
                           seed=s['seed'], n_init=s['n_init'], column=s['score'], feature_source=s['feature_source'],
                           device=device)
    return list(pool.filenames), res


def main(argv=None, scorer=score_and_partition):
    args = parse_args(argv)
    import config
    cfg = config.fromfile(args.config)
    s = settings(args, cfg)
    names, res = scorer(cfg, args, s)
    meta = dict(config=args.config, checkpoint=args.checkpoint, weights=s['weights'], score=s['score'], seed=s['seed'],
                num_clusters=s['num_clusters'], per_cluster=s['per_cluster'], feature_source=s['feature_source'],
                n_iter=int(res['n_iter']), inertia=float(res['inertia']))
    doc = document([os.path.basename(n) for n in names], [list(map(float, r)) for r in res['scores'].tolist()],
                   [int(l) for l in res['labels'].tolist()], res['clusters'], res['ranking'], meta)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(f"{len(names)} images, {s['num_clusters']} clusters, {sum(len(c) for c in res['clusters'])} selected "
          f"-> {args.out}")
    return doc


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
