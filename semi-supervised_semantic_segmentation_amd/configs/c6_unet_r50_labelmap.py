"""Config C6 on label maps: c6_unet_r50_multiclass with the labelled masks as [H, W] uint8 label maps instead of
19-channel one-hot floats, 5 % of the pixels void (label 255): cross-entropy with ignore_index + Lovasz-softmax with
ignore on the labelled batch, validation over the valid pixels only."""
from functools import partial

import torch

import losses
from data.synthetic import SyntheticSegDataset
from models.adapters import ListOutput
from models.encoders.resnet import resnet50_encoder
from models.unet import UNet

NUM_CLASSES = 19
IGNORE_LABEL = 255

common = dict(world_size=1, use_cpu=False, workers=8, output_dir='runs/c6_unet_r50_labelmap',
              num_classes=NUM_CLASSES, image_size=512, compute_dtype='bf16')
model = dict(model_fn=lambda: ListOutput(UNet(NUM_CLASSES, resnet50_encoder(), max_width=128,
                                              norm_layer=torch.nn.BatchNorm2d, train_upsampling=True)))
train = dict(print_freq=10, batch_size_per_worker=16, virtual_batch_size_multiplier=1, num_dataloader_workers=2,
             crop_size=512, gradient_clip_value=5.0, use_semi_supervised=True, mask_proportion_range=(0.45, 0.55),
             sigma_range=(8, 32), consistency_loss_weight=10, ema_model_alpha=0.99, confidence_threshold=0.97,
             consistency_activation='softmax', pretrained_checkpoint_path='', ignore_label=IGNORE_LABEL)
train['base_lr'] = 0.0001 * train['virtual_batch_size_multiplier'] / 4 * 9
train['loss'] = losses.CalculateLoss([{'loss_fn': losses.CrossEntropyLossWithLogits(ignore_index=IGNORE_LABEL),
                                       'weight': [0.5]},
                                      {'loss_fn': losses.LovaszSoftmaxLossWithLogits(ignore=IGNORE_LABEL),
                                       'weight': [0.5]}])
train['min_lr'] = train['base_lr'] * 0.001
train['optimizer'] = partial(torch.optim.SGD, lr=train['base_lr'], momentum=0.9, weight_decay=0.0005)
train['lr_scheduler'] = partial(torch.optim.lr_scheduler.CosineAnnealingWarmRestarts, T_0=300, T_mult=2,
                                eta_min=train['base_lr'] * 0.01, last_epoch=-1)
train['dataset'] = partial(SyntheticSegDataset, length=160, size=512, seed=1, num_classes=NUM_CLASSES,
                           label_map=True, void_fraction=0.05, ignore_label=IGNORE_LABEL)
train['unsupervised_dataset'] = partial(SyntheticSegDataset, length=320, size=512, seed=3, with_masks=False)
val = dict(batch_size_per_worker=16, num_dataloader_workers=2,
           dataset=partial(SyntheticSegDataset, length=32, size=512, seed=2, num_classes=NUM_CLASSES,
                           label_map=True, void_fraction=0.05, ignore_label=IGNORE_LABEL))
