"""Config C6 with ClassMix (Olsson et al. 2021) in place of CowMix: the mixing mask of the consistency branch follows
the teacher's own 19-class prediction on the first unlabelled batch -- per image, half of the classes its argmax map
holds (mixmasks.generate_classmix_masks_like, keys drawn on the device)."""
from c6_unet_r50_multiclass import common, model, train, val  # noqa: F401  (the rest of C6 unchanged; fromfile puts configs/ on the path)

common = dict(common, output_dir='runs/c6_unet_r50_classmix')
train = dict(train)
train['mix_mask'] = 'classmix'
