"""Config C2 with geometric consistency (the reference's plan, train.py:16-17): the student's consistency view is
rotated by up to +-15 degrees and rescaled by 0.75 .. 1.25 per sample (reversible_augmentations.RotateRescale, drawn on
the device), its prediction is warped back and compared with the teacher's on the pixels that stayed in the frame."""
from functools import partial

from c2_unet_r50 import common, model, train, val  # noqa: F401  (the rest of C2 unchanged; fromfile puts configs/ on the path)
from reversible_augmentations import RotateRescale

common = dict(common, output_dir='runs/c2_unet_r50_geo')
train = dict(train)
train['consistency_augmentation'] = partial(RotateRescale, 15, 0.75, 1.25)
