"""Host-side checks of the geometric consistency branch (no GPU): the affine matrices against the closed formulas, the
parameter ranges of RotateRescale, and the host-side argument validation of the new entry points."""
import ctypes
import math

import pytest
import torch

import geo_ref


def test_affine_mats_match_closed_formulas_and_invert():
    from ssseg import ops
    H, W = 19, 24
    mats, inv = ops.affine_mats([p[0] for p in geo_ref.PAIRS], [p[1] for p in geo_ref.PAIRS], H, W, 'cpu')
    assert mats.dtype == torch.float32 and tuple(mats.shape) == (len(geo_ref.PAIRS), 6)
    ref, ref_inv = geo_ref.mats64(geo_ref.PAIRS, H, W)
    assert float((mats.double() - ref).abs().max()) < 2e-6      # fp32 rounding of entries of magnitude < 32
    assert float((inv.double() - ref_inv).abs().max()) < 2e-6
    # theta = 0, s = 1 is exactly the identity
    assert mats[0].tolist() == [1, 0, 0, 0, 1, 0] and inv[0].tolist() == [1, 0, 0, 0, 1, 0]
    # A A^-1 = I as 3x3 homogeneous matrices (fp32-rounded entries, translations of magnitude < 64)
    row = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    for m, mi in zip(mats.double(), inv.double()):
        prod = torch.cat([m.reshape(2, 3), row]) @ torch.cat([mi.reshape(2, 3), row])
        assert float((prod - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5
    # at s = 1 the map is the rotation about the centre that ops.rotate uses
    th = math.radians(90.0)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    sx, sy = geo_ref.coords(ref[4:5], H, W)
    assert abs(float(sx[0, 3, 5]) - (math.cos(th) * (5 - cx) - math.sin(th) * (3 - cy) + cx)) < 1e-12
    assert abs(float(sy[0, 3, 5]) - (math.sin(th) * (5 - cx) + math.cos(th) * (3 - cy) + cy)) < 1e-12


def test_rotate_rescale_rejects_out_of_range_parameters():
    import reversible_augmentations as RA
    RA.RotateRescale(0, 1, 1)
    RA.RotateRescale(180, 0.25, 4, source='cpu')
    for bad in [(-1, 1, 1), (181, 1, 1), (10, 0.2, 1), (10, 1, 4.5), (10, 1.5, 1.2)]:
        with pytest.raises(ValueError):
            RA.RotateRescale(*bad)
    with pytest.raises(ValueError):
        RA.RotateRescale(10, 1, 1, source='host')
    aug = RA.RotateRescale(15, 0.75, 1.25)
    aug.set_params([17.5, -15.0], [0.8, 1.25])
    for bad in [([200.0], [1.0]), ([0.0], [0.1]), ([0.0], [5.0]), ([0.0, 1.0], [1.0])]:
        with pytest.raises(ValueError):
            aug.set_params(*bad)


def test_cpu_source_draws_angles_then_scales_within_range():
    import reversible_augmentations as RA
    from ssseg import ops
    aug = RA.RotateRescale(15, 0.75, 1.25, source='cpu')
    x = torch.zeros(8, 1, 9, 11)
    torch.manual_seed(5)
    mats, inv = aug._draw(x)
    torch.manual_seed(5)
    angles = (torch.rand(8) * 2 - 1) * 15
    scales = 0.75 + torch.rand(8) * 0.5
    ref, ref_inv = ops.affine_mats(angles, scales, 9, 11, 'cpu')
    assert torch.equal(mats, ref) and torch.equal(inv, ref_inv)
    assert float(angles.abs().max()) <= 15 and 0.75 <= float(scales.min()) and float(scales.max()) <= 1.25


def test_new_entry_points_validate_on_the_host():
    """null pointers -> SSSEG_EINVAL (-1), an unknown dtype code -> SSSEG_EUNSUPPORTED (-2); no device is touched"""
    from ssseg import native
    lib = native.lib()
    st = (ctypes.c_int64 * 4)(12, 4, 2, 1)
    one = ctypes.c_void_p(16)   # a non-null pointer that is never dereferenced: validation fails first
    assert lib.ssseg_affine_warp_fwd(None, None, None, 1, 1, 2, 2, st, st, 0, None, None) == -1
    assert lib.ssseg_affine_warp_fwd(one, one, None, 1, 1, 2, 2, st, st, 0, None, None) == -1
    assert lib.ssseg_affine_warp_fwd(one, one, one, 1, 1, 0, 2, st, st, 0, None, None) == -1
    assert lib.ssseg_affine_warp_fwd(one, one, one, 1, 1, 2, 2, None, st, 0, None, None) == -1
    assert lib.ssseg_affine_warp_fwd(one, one, one, 1, 1, 2, 2, st, st, 7, None, None) == -2
    assert lib.ssseg_affine_warp_bwd(None, None, None, None, 1, 1, 2, 2, st, st, 0, None) == -1
    assert lib.ssseg_affine_warp_bwd(one, one, one, None, 1, 1, 2, 2, st, st, 0, None) == -1
    assert lib.ssseg_affine_warp_bwd(one, one, one, one, 1, 1, 2, 2, st, st, 9, None) == -2
    d = ctypes.c_double
    assert lib.ssseg_affine_draw_dev(None, None, 2, 4, 4, d(15), d(0.75), d(1.25), 1, None, None) == -1
    assert lib.ssseg_affine_draw_dev(one, one, 2, 4, 4, d(15), d(0.75), d(1.25), 1, None, None) == -1
    assert lib.ssseg_affine_draw_dev(one, one, 0, 4, 4, d(15), d(0.75), d(1.25), 1, one, None) == -1
    assert lib.ssseg_affine_draw_dev(one, one, 2, 4, 4, d(15), d(1.25), d(0.75), 1, one, None) == -1
    f = ctypes.c_float
    assert lib.ssseg_consistency_w_fwd(None, None, None, 1, 1, 4, f(0.5), None, None, 0, None) == -1
    assert lib.ssseg_consistency_w_fwd(one, one, None, 1, 1, 4, f(0.5), one, one, 1 << 20, None) == -1
    assert lib.ssseg_consistency_w_bwd(None, None, None, 1, 1, 4, f(0.5), None, None, None, None) == -1
    assert lib.ssseg_consistency_w_bwd(one, one, None, 1, 1, 4, f(0.5), one, one, one, None) == -1


def test_augmentation_factory_is_called_once():
    import reversible_augmentations as RA
    import train
    made = []

    def factory():
        made.append(1)
        return RA.RotateRescale(15, 0.75, 1.25)
    tc = {'consistency_augmentation': factory}
    aug = train._consistency_augmentation(tc)
    assert train._consistency_augmentation(tc) is aug and made == [1]      # the factory is called once
    assert train._consistency_augmentation({}) is None
