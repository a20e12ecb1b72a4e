"""Config C6 with ClassMix as published (Olsson et al. 2021): ClassMix masks, and the student trained with
cross-entropy against the teacher's hard pseudo-labels, the whole unsupervised loss scaled by the fraction of pixels whose
teacher confidence passes confidence_threshold (ops.consistency_loss_ce, weighting 'batch')."""
from c6_unet_r50_classmix import common, model, train, val  # noqa: F401  (the rest of C6 unchanged; fromfile puts configs/ on the path)

common = dict(common, output_dir='runs/c6_unet_r50_classmix_ce')
train = dict(train)
train['consistency_loss'] = 'ce'
train['consistency_ce_weighting'] = 'batch'
