"""Config C6 with CutMix-Seg (French et al. 2020) and FixMatch's normalisation: CutMix boxes, and the student trained
with cross-entropy against the teacher's hard pseudo-labels on the pixels whose teacher confidence passes
confidence_threshold, divided by the number of all pixels (ops.consistency_loss_ce, weighting 'pixel': a step without a
confident pixel has a zero unsupervised loss, not 0/0)."""
from c6_unet_r50_multiclass import common, model, train, val  # noqa: F401  (the rest of C6 unchanged; fromfile puts configs/ on the path)

common = dict(common, output_dir='runs/c6_unet_r50_cutmix_ce')
train = dict(train)
train['mix_mask'] = 'cutmix'
train['consistency_loss'] = 'ce'
train['consistency_ce_weighting'] = 'pixel'
