"""Config C2 with CutMix (French et al. 2020) in place of CowMix: one random box per image whose area is the
mask_proportion_range share of it (mixmasks.generate_cutmix_masks_like, parameters drawn on the device)."""
from c2_unet_r50 import common, model, train, val  # noqa: F401  (the rest of C2 unchanged; fromfile puts configs/ on the path)

common = dict(common, output_dir='runs/c2_unet_r50_cutmix')
train = dict(train)
train['mix_mask'] = 'cutmix'
