"""c6_unet_r50_labelmap with a Cityscapes-style validation set: the model is trained on 512 x 512 crops and validated
on 1024 x 1024 images by sliding-window inference (ssseg.sliding.SlidingWindowInference: crops of the training size at
stride 341, overlaps averaged, the fused logit map at the image's own size going to the loss and the metrics).  The
network sees [window_batch, 3, 512, 512] whatever the validation image size is."""
from functools import partial

from c6_unet_r50_labelmap import IGNORE_LABEL, NUM_CLASSES, common, model, train  # noqa: F401  (fromfile puts configs/ on the path)
from data.synthetic import SyntheticSegDataset

common = dict(common, output_dir='runs/c6_unet_r50_labelmap_sliding')
val = dict(batch_size_per_worker=2, num_dataloader_workers=2,
           dataset=partial(SyntheticSegDataset, length=8, size=1024, seed=2, num_classes=NUM_CLASSES,
                           label_map=True, void_fraction=0.05, ignore_label=IGNORE_LABEL),
           sliding_window=dict(crop_size=512, stride=341, scales=(1.0,), flip=False, weighting='uniform',
                               window_batch=8))
