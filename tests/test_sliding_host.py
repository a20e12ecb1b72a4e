"""CPU: sliding.window_plan's rule and the host restatement of the fusion (tests/sliding_ref.py)."""
import itertools

import pytest
import torch

import sliding_ref as R
from ssseg import sliding

# (H, W), crop, stride: larger than the crop, not a multiple of the stride, smaller than the crop (one or both axes),
# equal to the crop, stride == crop, a non-square crop, one window per axis short of an exact fit
CASES = [((40, 72), (32, 32), (24, 24)), ((37, 53), (32, 32), (24, 24)), ((20, 50), (32, 32), (24, 24)),
         ((20, 20), (32, 32), (24, 24)), ((32, 32), (32, 32), (24, 24)), ((64, 64), (32, 32), (32, 32)),
         ((65, 64), (32, 32), (32, 32)), ((40, 72), (32, 64), (24, 32)), ((37, 53), (32, 64), (32, 24)),
         ((1024, 2048), (512, 512), (341, 341)), ((1, 1), (32, 32), (24, 24)), ((33, 96), (32, 32), (1, 32))]
IDS = [f'{h}x{w}-c{c[0]}x{c[1]}-s{s[0]}x{s[1]}' for (h, w), c, s in CASES]


def count_map(H, W, crop, plan):
    frame = (max(H, crop[0]), max(W, crop[1]))
    cnt = torch.zeros(frame, dtype=torch.int64)
    for y0, x0 in plan:
        cnt[y0:y0 + crop[0], x0:x0 + crop[1]] += 1
    return cnt


@pytest.mark.parametrize('size,crop,stride', CASES, ids=IDS)
def test_plan_covers_the_frame_and_stays_inside(size, crop, stride):
    H, W = size
    plan = sliding.window_plan(H, W, crop, stride)
    fh, fw = max(H, crop[0]), max(W, crop[1])
    assert all(0 <= y0 and y0 + crop[0] <= fh and 0 <= x0 and x0 + crop[1] <= fw for y0, x0 in plan)
    assert int(count_map(H, W, crop, plan).min()) >= 1                      # every pixel of the frame is covered
    assert plan == sorted(plan) and len(set(plan)) == len(plan)             # row-major, no window twice
    ys, xs = sorted({y for y, _ in plan}), sorted({x for _, x in plan})
    assert plan == list(itertools.product(ys, xs))
    # the rule, axis by axis: i * stride until the last window, which ends at the frame's edge
    for origins, f, c, s in ((ys, fh, crop[0], stride[0]), (xs, fw, crop[1], stride[1])):
        assert len(origins) == -(-(f - c) // s) + 1
        assert origins[:-1] == [i * s for i in range(len(origins) - 1)]
        assert origins[-1] == f - c
    assert plan == R.plan(H, W, crop, stride)


@pytest.mark.parametrize('size,crop,stride', CASES[:9], ids=IDS[:9])
def test_count_map_equals_brute_force(size, crop, stride):
    H, W = size
    plan = sliding.window_plan(H, W, crop, stride)
    fh, fw = max(H, crop[0]), max(W, crop[1])
    brute = torch.tensor([[sum(y0 <= y < y0 + crop[0] and x0 <= x < x0 + crop[1] for y0, x0 in plan)
                           for x in range(fw)] for y in range(fh)])
    assert torch.equal(count_map(H, W, crop, plan), brute)
    # the restatement's weight map with uniform weights is that count, for every image of the batch
    outs = [torch.zeros(1, *crop)] * (2 * len(plan))
    _, wsum = R.fuse(outs, R.rows(2, H, W, crop, stride), 2, (fh, fw), crop, 'none')
    assert torch.equal(wsum, brute.double().expand(2, fh, fw))


def test_ints_and_pairs_and_defaults():
    assert sliding.window_plan(40, 72, 32, 24) == sliding.window_plan(40, 72, (32, 32), (24, 24))
    assert sliding.window_plan(20, 20, 32, 24) == [(0, 0)]
    assert sliding.window_plan(32, 32, 32, 24) == [(0, 0)]
    assert sliding.window_plan(64, 64, 32, 32) == [(0, 0), (0, 32), (32, 0), (32, 32)]
    assert sliding.window_plan(40, 72, 32, 24) == [(0, 0), (0, 24), (0, 40), (8, 0), (8, 24), (8, 40)]
    assert len(sliding.window_plan(1024, 2048, 512, 341)) == 3 * 6
    with pytest.raises(ValueError):
        sliding.window_plan(0, 5, 32, 24)
    with pytest.raises(ValueError):
        sliding.window_plan(5, 5, 32, 0)
    s = sliding.SlidingWindowInference(torch.nn.Identity(), 512)
    assert s.stride == (342, 342) and s.crop == (512, 512)                  # 2/3 of the crop, rounded up
    assert sliding.SlidingWindowInference(torch.nn.Identity(), (32, 64)).stride == (22, 43)


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('wb', [1, 4])
def test_window_list_order_and_padding(flip, wb):
    s = sliding.SlidingWindowInference(torch.nn.Identity(), 32, stride=24, flip=flip, window_batch=wb)
    rows = s.windows(3, 40, 72)
    assert rows == R.rows(3, 40, 72, (32, 32), (24, 24), flip, wb)
    real = [r for r in rows if not r[3] & R.NULL]
    assert len(real) == 3 * 6 * (2 if flip else 1) and len(rows) % wb == 0 and len(rows) - len(real) < wb
    assert rows[:len(real)] == real                                          # the null windows trail
    assert [r[0] for r in real[:18]] == [b for b in range(3) for _ in range(6)]
    if flip:
        assert [r[:3] for r in real[18:]] == [r[:3] for r in real[:18]] and all(r[3] == R.MIRROR for r in real[18:])


@pytest.mark.parametrize('size,crop,stride', CASES[:9], ids=IDS[:9])
def test_restatement_of_a_pointwise_model_is_the_whole_image_function(size, crop, stride):
    """Window by window, non-mirrored: cut the crop (zero padding), apply the pointwise function, fuse.  With uniform
    weights every overlap averages equal integers, so the fused map equals the function of the whole image exactly."""
    H, W = size
    B, C = 2, 5
    img, w = R.integer_image(B, H, W, seed=H + W), R.mix_weights(C)
    fh, fw = max(H, crop[0]), max(W, crop[1])
    padded = torch.zeros(B, 3, fh, fw, dtype=torch.float64)
    padded[:, :, :H, :W] = img
    table = R.rows(B, H, W, crop, stride)
    outs = [R.pointwise(padded[b:b + 1, :, y0:y0 + crop[0], x0:x0 + crop[1]], w)[0] for b, y0, x0, _ in table]
    fused, wsum = R.fused_map([(outs, table, (H, W))], B, (H, W), crop, 'none')
    assert torch.equal(fused, R.pointwise(img, w))
    assert int(wsum.min()) >= 1


def test_restatement_unmirrors_and_ignores_null_windows():
    H, W, crop, stride = 37, 53, (32, 32), (24, 24)
    img, w = R.integer_image(1, H, W, seed=3), R.mix_weights(4)
    table = R.rows(1, H, W, crop, stride, flip=True, window_batch=5)
    assert any(f & R.NULL for *_, f in table)
    outs = []
    for b, y0, x0, f in table:
        c = img[b:b + 1, :, y0:y0 + 32, x0:x0 + 32]
        o = R.pointwise(c.flip(-1) if f & R.MIRROR else c, w)[0]
        outs.append(torch.full_like(o, 1e30) if f & R.NULL else o)
    fused, _ = R.fused_map([(outs, table, (H, W))], 1, (H, W), crop, 'none')
    assert torch.equal(fused, R.pointwise(img, w))


def test_sliding_config():
    import os

    import config
    from conftest import PKG
    cfg = config.fromfile(os.path.join(PKG, 'configs', 'c6_unet_r50_labelmap_sliding.py'))
    base = config.fromfile(os.path.join(PKG, 'configs', 'c6_unet_r50_labelmap.py'))
    sw = cfg['val']['sliding_window']
    assert 'sliding_window' not in base['val']
    assert sw['crop_size'] == cfg['train']['crop_size'] == 512 and sw['stride'] == 341
    kw = cfg['val']['dataset'].keywords
    assert kw['size'] == 1024 and kw['label_map'] is True and kw['ignore_label'] == 255 and kw['num_classes'] == 19
    assert cfg['train']['loss'] is not None and cfg['train']['ignore_label'] == 255
    # the keys are the constructor's: the runner builds from them as train.validate builds it
    s = sliding.SlidingWindowInference(torch.nn.Identity(), activation='none', **sw)
    assert len(s.windows(2, 1024, 1024)) == 2 * 9 + 6 and s.window_batch == 8
