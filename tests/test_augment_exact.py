"""Per-pixel, tie-aware tests of the device augmentation kernels (csrc/augment.hip: ssseg_aug_warp, ssseg_aug_color,
ssseg_aug_blur, ssseg_aug_iso_finish) and of DeviceAugment as their composition.  The case tables, the expected values
and the rule (decided elements bit-equal to the fp64 oracle, undecided ones one of the two neighbouring outcomes, capped
shares) are tests/augment_cases.py; tests/test_augment_exact_host.py shows on the CPU that the caps hold and that the
comparators reject the listed mistakes on these very tables.  Every test prints its worst observed / eps (the largest
distance from a rounding boundary at which the device still rounded the other way, over eps; above 1 fails) and its
undecided share."""
import ctypes

import numpy as np
import pytest
import torch

import augment_cases as A

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
PAD = 64


def _guarded(shape, dev, dtype=torch.float32):
    """a buffer of `shape` with PAD sentinels before and after it: (whole buffer, the view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[PAD:PAD + n].view(*shape)


def _guards_untouched(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


def _records(cls, dicts, dev):
    arr = (cls * len(dicts))()
    for rec, d in zip(arr, dicts):
        for k, v in d.items():
            if isinstance(v, (list, tuple)):
                getattr(rec, k)[:] = v
            else:
                setattr(rec, k, v)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


# ---- warp ------------------------------------------------------------------------------------------------------------
def _run_warp(case, dev):
    """both layouts of one case: (levels [n,Ho,Wo,3], mask [n,Cm,Ho,Wo] or None, ToFloat image [n,3,Ho,Wo])"""
    from data import device_augment as DA
    from ssseg import native as N
    n, H, W, _ = case['img'].shape
    Ho, Wo = case['Ho'], case['Wo']
    d_p = _records(DA.WarpParams, case['params'], dev)
    d_img = torch.from_numpy(case['img']).to(dev)
    d_g, d_f = torch.from_numpy(case['gmaps']).to(dev), torch.from_numpy(case['fields']).to(dev)
    ob, out = _guarded((n, Ho, Wo, 3), dev)
    fb, out01 = _guarded((n, 3, Ho, Wo), dev)
    d_mask = mb = om = None
    Cm = 0
    if case['mask'] is not None:
        Cm = case['mask'].shape[3]
        d_mask = torch.from_numpy(case['mask']).to(dev)
        mb, om = _guarded((n, Cm, Ho, Wo), dev)
    N.call('ssseg_aug_warp', N.dev_ptr(d_img), N.dev_ptr(d_mask), Cm, n, H, W, N.dev_ptr(out), N.dev_ptr(om), Ho, Wo,
           N.dev_ptr(d_p), N.dev_ptr(d_g), N.dev_ptr(d_f), 0, N.stream())
    N.call('ssseg_aug_warp', N.dev_ptr(d_img), None, 0, n, H, W, N.dev_ptr(out01), None, Ho, Wo, N.dev_ptr(d_p),
           N.dev_ptr(d_g), N.dev_ptr(d_f), 1, N.stream())
    torch.cuda.synchronize()
    assert _guards_untouched(ob) and _guards_untouched(fb) and (mb is None or _guards_untouched(mb)), case['name']
    return out.cpu().numpy(), None if om is None else om.cpu().numpy(), out01.cpu().numpy()


def _check_warp_case(case, dev):
    exp = A.warp_expected(case)
    got, gm, g01 = _run_warp(case, dev)
    # ToFloat layout: float(level) * (1.f / 255.f) of the same levels, bit for bit
    assert np.array_equal(g01, A.to_float(got).transpose(0, 3, 1, 2)), case['name']
    return A.check_warp(case, exp, got, gm)


def test_warp_exact(hip_device):
    """the cases that are exact by construction: every element of image and mask equal, in both layouts (the image of
    the optical case by the rule: its bilinear weights are multiples of 2^-17)"""
    worst = share = 0.0
    cases = A.warp_exact_cases()
    for case in cases:
        r, s, sm = _check_warp_case(case, hip_device)
        assert sm == 0.0
        worst, share = max(worst, r), max(share, s)
    print(f'warp exact: {len(cases)} cases equal; optical image: worst observed / eps {worst:.3f}, undecided share {share:.5f}')


def test_warp_general(hip_device):
    for case in A.warp_general_cases():
        r, s, sm = _check_warp_case(case, hip_device)
        print(f'warp {case["name"]}: worst observed / eps {r:.3f}, undecided share image {s:.5f} mask {sm:.5f}')


# ---- colour ----------------------------------------------------------------------------------------------------------
def _run_color(imgs, recs, dev):
    from data import device_augment as DA
    from ssseg import native as N
    n, H, W, _ = imgs.shape
    d_p = _records(DA.ColorParams, recs, dev)
    buf, x = _guarded(imgs.shape, dev)
    x.copy_(torch.from_numpy(imgs))
    N.call('ssseg_aug_color', N.dev_ptr(x), n, H, W, N.dev_ptr(d_p), N.stream())
    torch.cuda.synchronize()
    assert _guards_untouched(buf)
    return x.cpu().numpy()


def test_color_lattice(hip_device):
    lat, recs = A.color_lattice(), A.color_records()
    got = _run_color(np.broadcast_to(lat, (len(recs),) + lat.shape).copy(), [p for _, p, _ in recs], hip_device)
    worst = share = 0.0
    for i, (name, p, exact) in enumerate(recs):
        r, s = A.check_color(got[i], A.color_expected(lat, p), exact, name)
        worst, share = max(worst, r), max(share, s)
    print(f'colour lattice: {len(recs)} records, worst observed / eps {worst:.3f}, largest undecided share {share:.5f}')


def test_color_second_grid_round(hip_device):
    img, p = A.color_big()
    got = _run_color(img[None], [p], hip_device)
    r, s = A.check_color(got[0], A.color_expected(img, p), False, '513 x 512')
    print(f'colour 513 x 512: worst observed / eps {r:.3f}, undecided share {s:.5f}')


# ---- blur ------------------------------------------------------------------------------------------------------------
def test_blur(hip_device):
    from ssseg import native as N
    worst = share = 0.0
    cases = A.blur_cases()
    for case in cases:
        n, H, W, C = case['x'].shape
        xb, x = _guarded(case['x'].shape, hip_device)
        tb, tmp = _guarded(case['x'].shape, hip_device)
        x.copy_(torch.from_numpy(case['x']))
        d_r, d_w = torch.from_numpy(case['radius']).to(hip_device), torch.from_numpy(case['weights']).to(hip_device)
        N.call('ssseg_aug_blur', N.dev_ptr(x), N.dev_ptr(tmp), n, H, W, C, N.dev_ptr(d_r), N.dev_ptr(d_w), A.WMAX,
               case['sym'], case['round8'], N.stream())
        torch.cuda.synchronize()
        assert _guards_untouched(xb) and _guards_untouched(tb), case['name']
        r, s = A.check_blur(case, A.blur_expected(case), x.cpu().numpy())
        worst, share = max(worst, r), max(share, s)
    print(f'blur: {len(cases)} cases, worst observed / eps {worst:.3f}, largest undecided share {share:.5f}')


# ---- ISO noise / ToFloat -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', (0, 1, 2))
def test_iso_finish(hip_device, which):
    from data import device_augment as DA
    from ssseg import native as N
    case = A.iso_cases()[which]
    name, img, recs, seed = case
    n, H, W, _ = img.shape
    d_p = _records(DA.ColorParams, recs, hip_device)
    x = torch.from_numpy(img).to(hip_device)
    ob, out = _guarded((n, 3, H, W), hip_device)
    sb, st = _guarded((n, 2), hip_device, torch.float64)
    N.call('ssseg_aug_iso_finish', N.dev_ptr(x), N.dev_ptr(out), n, H, W, N.dev_ptr(d_p), N.dev_ptr(st), seed, N.stream())
    torch.cuda.synchronize()
    assert _guards_untouched(ob) and _guards_untouched(sb)
    exp = A.iso_expected(case)
    stats = st.cpu().numpy()
    for i, e in enumerate(exp):
        if e['off']:
            assert (stats[i] == 0).all()                         # zeroed by the launcher, skipped by the kernel
    r, s, sc, rs = A.check_iso(case, exp, out.cpu().numpy(), stats)
    print(f'iso {name}: worst observed / eps {r:.3f}, undecided share image {s:.4f} counts {sc:.6f}, luminance sums '
          f'error / bound {rs:.3f}; lambda {[round(e["lam"], 3) for e in exp if not e["off"]]}')


# ---- composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', A.COMPOSITION['seeds'])
def test_train_is_the_composition_of_the_kernels(hip_device, seed):
    """DeviceAugment.train / .unsupervised with every stage on equal this test's own sequence of kernel calls, built
    from a second DeviceAugment with the same seed: draw(), then the getrandbits(64) values in the order train takes
    them (the field seed if any sample is elastic, then the ISO seed).  Pins the stage order, sym / round8 per call, the
    sqrt(alpha) taps on both passes of the field blur, the field indices and the layouts."""
    import math
    from data import device_augment as DA
    from ssseg import native as N
    cfg = A.COMPOSITION
    S, (H, W), n = cfg['S'], cfg['hw'], cfg['n']
    rng = np.random.default_rng(seed)
    dev = hip_device
    img = torch.from_numpy(rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(rng.integers(0, 256, size=(n, H, W, 2), dtype=np.uint8)).to(dev)
    aug = DA.DeviceAugment(S, seed=seed, **cfg['kw'])
    x, m = aug.train(img, mask)
    u = aug.unsupervised(img)
    torch.cuda.synchronize()

    ref = DA.DeviceAugment(S, seed=seed, **cfg['kw'])
    up = lambda a: ref._upload(a, dev)      # noqa: E731
    warp, color, gmaps, radius, weights, nf = ref.draw(n, H, W, True)
    assert nf >= 1 and sorted(w.field for w in warp if w.distort == 1) == list(range(nf)) and (radius > 0).all()
    d_warp, d_color, d_gmaps = up(warp), up(color), up(gmaps)
    stream = N.stream()
    fields = torch.empty((nf, S, S, 2), device=dev)
    alpha, sigma, _ = ref.elastic
    N.call('ssseg_aug_uniform_field', N.dev_ptr(fields), fields.numel(), ref.rng.getrandbits(64), stream)
    taps = DA.scipy_gaussian_taps(sigma)
    fr = np.full(nf, len(taps) // 2, np.int32)
    fw = np.zeros((nf, DA.WMAX), np.float32)
    fw[:, :len(taps)] = taps * math.sqrt(alpha)
    d_fr, d_fw, ftmp = up(fr), up(fw), torch.empty_like(fields)
    N.call('ssseg_aug_blur', N.dev_ptr(fields), N.dev_ptr(ftmp), nf, S, S, 2, N.dev_ptr(d_fr), N.dev_ptr(d_fw), DA.WMAX, 1,
           0, stream)
    lv = torch.empty((n, S, S, 3), device=dev)
    rm = torch.empty((n, 2, S, S), device=dev)
    N.call('ssseg_aug_warp', N.dev_ptr(img), N.dev_ptr(mask), 2, n, H, W, N.dev_ptr(lv), N.dev_ptr(rm), S, S,
           N.dev_ptr(d_warp), N.dev_ptr(d_gmaps), N.dev_ptr(fields), 0, stream)
    N.call('ssseg_aug_color', N.dev_ptr(lv), n, S, S, N.dev_ptr(d_color), stream)
    d_r, d_w, tmp = up(radius), up(weights), torch.empty_like(lv)
    N.call('ssseg_aug_blur', N.dev_ptr(lv), N.dev_ptr(tmp), n, S, S, 3, N.dev_ptr(d_r), N.dev_ptr(d_w), DA.WMAX, 0, 1,
           stream)
    rx = torch.empty((n, 3, S, S), device=dev)
    st = torch.empty((n, 2), device=dev, dtype=torch.float64)
    N.call('ssseg_aug_iso_finish', N.dev_ptr(lv), N.dev_ptr(rx), n, S, S, N.dev_ptr(d_color), N.dev_ptr(st),
           ref.rng.getrandbits(64), stream)
    uwarp = ref.draw(n, H, W, False)[0]
    d_uwarp = up(uwarp)
    ru = torch.empty((n, 3, S, S), device=dev)
    N.call('ssseg_aug_warp', N.dev_ptr(img), None, 0, n, H, W, N.dev_ptr(ru), None, S, S, N.dev_ptr(d_uwarp), None, None,
           1, stream)
    torch.cuda.synchronize()
    assert ctypes.sizeof(DA.WarpParams) * n == d_warp.numel()
    assert torch.equal(x, rx) and torch.equal(m, rm) and torch.equal(u, ru)
    assert float(x.std()) > 0.05 and float(u.std()) > 0.05 and not torch.equal(x, u)
    print(f'seed {seed}: train and unsupervised equal their kernel sequences; {nf} elastic samples, kinds '
          f'{[w.distort for w in warp]}, radii {radius.tolist()}')
