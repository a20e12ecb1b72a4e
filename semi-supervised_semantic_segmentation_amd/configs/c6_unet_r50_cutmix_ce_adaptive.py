"""c6_unet_r50_cutmix_ce with self-adaptive per-class confidence thresholds (FreeMatch, Wang et al. 2023) in the place of
the fixed confidence_threshold: the thresholds start at 1 / C, rise with the teacher's mean confidence and are scaled
down for the classes the teacher predicts with low probability (ops.AdaptiveThreshold; the state lives on the device,
is updated in every semi-supervised step and is saved in the checkpoint)."""
from c6_unet_r50_cutmix_ce import common, model, train, val  # noqa: F401  (fromfile puts configs/ on the path)

common = dict(common, output_dir='runs/c6_unet_r50_cutmix_ce_adaptive')
train = dict(train)
train['confidence_threshold_mode'] = 'adaptive'
train['confidence_threshold_momentum'] = 0.999
