"""Every device-side random draw against the host Philox restatement of tests/philox_ref.py, with explicit seeds and
counters: csrc/cowmix.hip (normals, p, sigma), warp.hip (affine views), mixmask.hip (ClassMix keys, CutMix params),
pool.hip (dropout) and augment.hip (ElasticTransform field, ISO hue noise), then the production CowMix path end to end.
Integer-valued outputs are compared bit for bit; the others within the bounds derived in philox_ref's docstring.  Every
test prints its largest error / bound ratio.  tests/test_device_rng_host.py shows that the comparators used here reject
nine rounds, exchanged sin / cos, a wrong stream word and a dropped carry."""
import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
PAD = 4


def _counter(dev, value):
    """a device counter (int64, read by the kernels as unsigned) holding value mod 2^64"""
    v = int(value) % 2 ** 64
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device=dev)


def _value(ctr):
    return int(ctr.item()) % 2 ** 64


def _padded(n, dev, dtype=torch.float32):
    """n elements followed by PAD sentinels; (whole buffer, the view of the first n)"""
    buf = torch.full((n + PAD,), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[:n]


def _pad_untouched(buf):
    return bool((buf[-PAD:] == SENTINEL).all())


# ---- 1. exact integer checks -----------------------------------------------------------------------------------------
def _mixmask(dev, B, C, seed, ctr, keys=True, params=True):
    from ssseg import native as N
    kb, k = _padded(B * C, dev, torch.int32)
    pb, p = _padded(B * 4, dev)
    N.call('ssseg_mixmask_draw_dev', N.dev_ptr(k) if keys else None, N.dev_ptr(p) if params else None, B, C, seed,
           N.dev_ptr(ctr), N.stream())
    torch.cuda.synchronize()
    assert _pad_untouched(kb) and _pad_untouched(pb)
    return k.view(B, C).cpu().numpy(), p.view(B, 4).cpu().numpy()


@pytest.mark.parametrize('start', P.DEV_COUNTERS)
@pytest.mark.parametrize('seed', P.SEEDS)
def test_mixmask_keys_and_params(hip_device, seed, start):
    """ClassMix keys (stream 3) and CutMix params (stream 4), bit for bit: a keys-only call, a params-only call and a
    call for both, one after the other on the advancing counter -- an output that is not asked for keeps its counters,
    the advance is B (ceil(C/4) + 1) either way.  The last shape is a second grid-stride round."""
    for B, C in P.MIXMASK_SHAPES:
        ctr, at = _counter(hip_device, start), start
        for keys, params in ((True, False), (False, True), (True, True)):
            k, p = _mixmask(hip_device, B, C, seed, ctr, keys, params)
            rk, rp, adv = P.mixmask_draw(B, C, seed, at)
            assert adv == B * (-(-C // 4) + 1)
            if keys:
                P.check_exact(k, rk, f'keys B={B} C={C} counter {at}')
            else:
                assert (k == int(SENTINEL)).all()
            if params:
                P.check_exact(p, rp, f'params B={B} C={C} counter {at}')
            else:
                assert (p == SENTINEL).all()
            at += adv
            assert _value(ctr) == at % 2 ** 64
    B, C = P.MIXMASK_LARGE
    ctr = _counter(hip_device, start)
    k, p = _mixmask(hip_device, B, C, seed, ctr)
    rk, rp, adv = P.mixmask_draw(B, C, seed, start)
    P.check_exact(k, rk, f'keys B={B} C={C}')
    P.check_exact(p, rp, f'params B={B} C={C}')
    assert _value(ctr) == (start + adv) % 2 ** 64
    print(f'seed {seed:#x} counter {start:#x}: keys and params equal at {P.MIXMASK_SHAPES + (P.MIXMASK_LARGE,)}')


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16, torch.float16))
@pytest.mark.parametrize('seed', P.SEEDS)
def test_dropout_mask(hip_device, seed, dtype):
    """ssseg_dropout (host offset) and ssseg_dropout_dev (device counter) on x = 1: the mask is philox_ref.dropout_mask,
    a kept 1 is the fp32 quotient 1 / (1 - p) rounded to the type, the two entry points agree bit for bit, the counter
    is left as it was (ssseg_rng_take advances it).  No second grid-stride round: dropout's grid cap is 2^20 blocks of
    256 threads, so a second round needs 2^30 elements, which is left out."""
    from ssseg import native as N
    offsets = tuple(dict.fromkeys(P.HOST_OFFSETS + P.DEV_COUNTERS))
    kept = 0
    for n in P.DROPOUT_SIZES:
        x = torch.ones(n, device=hip_device, dtype=dtype)
        for p in P.DROPOUT_PS:
            scale = torch.tensor(float(P.dropout_scale(p)), dtype=torch.float32).to(dtype)
            for off in offsets:
                hb, yh = _padded(n, hip_device, dtype)
                db, yd = _padded(n, hip_device, dtype)
                ctr = _counter(hip_device, off)
                N.call('ssseg_dropout', N.dev_ptr(x), N.dev_ptr(yh), n, float(p), seed, off, N.dt_code(x), N.stream())
                N.call('ssseg_dropout_dev', N.dev_ptr(x), N.dev_ptr(yd), n, float(p), seed, N.dev_ptr(ctr), N.dt_code(x),
                       N.stream())
                torch.cuda.synchronize()
                assert _pad_untouched(hb) and _pad_untouched(db) and _value(ctr) == off
                assert torch.equal(yh, yd), (n, p, off)
                y = yh.cpu()
                what = f'dropout {dtype} n={n} p={p} offset {off:#x}'
                P.check_exact((y != 0).numpy(), P.dropout_mask(n, p, seed, off), what)
                assert bool(((y == 0) | (y == scale)).all()), (what, float(scale))
                kept += int((y != 0).sum())
    print(f'seed {seed:#x} {dtype}: masks equal at n {P.DROPOUT_SIZES} p {P.DROPOUT_PS} offsets {offsets}; {kept} kept')


def test_dropout_backward_regenerates_the_mask(hip_device):
    """snn.Dropout with its counter at 2^32 - 3 (the carry falls inside the call): the forward's mask is the host's,
    the counter ends at the documented advance, and the backward -- after another forward has moved the counter on --
    regenerates the forward's mask from its snapshot."""
    from ssseg import nn as snn
    seed, start, p = P.SEEDS[1], 2 ** 32 - 3, 0.5
    old = snn._DROP['seed']
    try:
        snn._DROP['seed'] = seed
        x = torch.ones(1, 8, 3, 3, device=hip_device, dtype=snn.compute_dtype())
        x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        n = x.numel()
        ctr = snn.dropout_counter(x.device)
        ctr.fill_(start)
        d = snn.Dropout(p).train()
        y = d(x)
        assert _value(ctr) == start + n // 4 + 1
        y2 = d(x)
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
    finally:
        snn._DROP['seed'] = old
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1).float().cpu()       # noqa: E731  (memory order)
    P.check_exact((flat(y) != 0).numpy(), P.dropout_mask(n, p, seed, start), 'forward')
    P.check_exact((flat(y2) != 0).numpy(), P.dropout_mask(n, p, seed, start + n // 4 + 1), 'second forward')
    assert torch.equal(x.grad, y) and not torch.equal(y, y2)
    assert bool(((flat(y) == 0) | (flat(y) == 2.0)).all())


@pytest.mark.parametrize('seed', P.SEEDS)
def test_uniform_field(hip_device, seed):
    """the ElasticTransform displacement noise 2 u01(c0) - 1 (stream 0xe1a5, counter i), bit for bit; the last size
    is a second grid-stride round with a tail"""
    from ssseg import native as N
    for n in P.FIELD_SIZES:
        buf, f = _padded(n, hip_device)
        N.call('ssseg_aug_uniform_field', N.dev_ptr(f), n, seed, N.stream())
        torch.cuda.synchronize()
        assert _pad_untouched(buf)
        P.check_exact(f.cpu().numpy(), P.uniform_field(n, seed), f'uniform field n={n}')
    print(f'seed {seed:#x}: uniform field equal at n {P.FIELD_SIZES}')


def _cowmix_draw(dev, B, HW, ranges, seed, off, device_counter):
    from ssseg import native as N
    pb, p = _padded(B, dev)
    sb, s = _padded(B, dev)
    zb, z = _padded(B * HW, dev)
    args = (N.dev_ptr(p), N.dev_ptr(s), N.dev_ptr(z), B, HW, float(ranges[0]), float(ranges[1]), float(ranges[2]),
            float(ranges[3]), seed)
    if device_counter:
        ctr = _counter(dev, off)
        N.call('ssseg_cowmix_draw_dev', *args, N.dev_ptr(ctr), N.stream())
    else:
        N.call('ssseg_cowmix_draw', *args, off, N.stream())
    torch.cuda.synchronize()
    assert _pad_untouched(pb) and _pad_untouched(sb) and _pad_untouched(zb)
    if device_counter:
        assert _value(ctr) == (off + P.cowmix_advance(B, HW)) % 2 ** 64 and P.cowmix_advance(B, HW) == B + -(-B * HW // 4) + 1
    return p.cpu().numpy(), s.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize('seed', P.SEEDS)
def test_cowmix_draw(hip_device, seed):
    """ssseg_cowmix_draw (host offset) and ssseg_cowmix_draw_dev (device counter): with the proportion range (0, 1) p is
    float(c0 >> 8) 2^-24 of stream 1 exactly; with the suite's ranges p is within 1 ulp, sigma within
    2^-23 (4 + 2 |a|) and inside its range, and the noise (stream 0, counters from offset + B) within the normals'
    bound; the device counter ends at offset + B + ceil(B HW / 4) + 1."""
    worst = dict(p=0.0, sigma=0.0, noise=0.0)
    HW = P.COWMIX_HW
    for B in P.COWMIX_BATCHES:
        for dev_ctr, offsets in ((False, P.HOST_OFFSETS), (True, P.DEV_COUNTERS)):
            for off in offsets:
                what = f'B={B} {"device counter" if dev_ctr else "host offset"} {off:#x}'
                p, _, _ = _cowmix_draw(hip_device, B, HW, (0, 1, 1, 6), seed, off, dev_ctr)
                P.check_exact(p, P.cowmix_draw(B, HW, (0, 1, 1, 6), seed, off)['p_unit'], 'p (0, 1) ' + what)
                for _, rng in P.END_TO_END:
                    p, s, z = _cowmix_draw(hip_device, B, HW, rng, seed, off, dev_ctr)
                    ref = P.cowmix_draw(B, HW, rng, seed, off)
                    worst['p'] = max(worst['p'], P.check_ulp(p, ref['p'], f'p {rng} {what}'))
                    worst['sigma'] = max(worst['sigma'], P.check_sigma(s, ref['sigma'], ref['a'], rng[2], rng[3],
                                                                       f'sigma {rng} {what}'))
                    worst['noise'] = max(worst['noise'], P.check_normals(z, ref['noise'], ref['rad'], f'noise {what}'))
    print(f'seed {seed:#x}: largest error / bound: p {worst["p"]:.3f} (of 1 ulp), sigma {worst["sigma"]:.3f}, '
          f'noise {worst["noise"]:.3f}')


# ---- 2. checks with derived bounds -----------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', P.HOST_OFFSETS)
@pytest.mark.parametrize('seed', P.SEEDS)
def test_normals(hip_device, seed, offset):
    """normal_kernel through ops.normal_: |z_dev - z_ref| <= 2^-21 (|z_ref| + rad_ref), |z| <= 5.89, nothing written
    past n; the last size is a second grid-stride round (2^20 + 2 counters on 4096 x 256 threads) with a tail."""
    from ssseg import ops
    worst = 0.0
    for n in P.NORMAL_SIZES:
        buf, out = _padded(n, hip_device)
        ops.normal_(out, seed, offset)
        torch.cuda.synchronize()
        assert _pad_untouched(buf)
        z, rad = P.normals(n, seed, offset, with_rad=True)
        r = P.check_normals(out.cpu().numpy(), z, rad, f'normals n={n} seed {seed:#x} offset {offset:#x}')
        worst = max(worst, r)
    print(f'seed {seed:#x} offset {offset:#x}: normals, largest error / bound {worst:.3f} at n {P.NORMAL_SIZES}')


@pytest.mark.parametrize('start', P.DEV_COUNTERS)
@pytest.mark.parametrize('seed', P.SEEDS)
def test_affine_draw(hip_device, seed, start):
    """ssseg_affine_draw_dev (stream 2): theta and s restated in fp32 from the Philox words, the matrices through
    geo_ref.mats64 -- rotation and scale entries within 1 fp32 ulp, translations within 2^-23 max(1, cx, cy); B = 300 is
    past the block's 256 threads; the counter ends at start + B."""
    from ssseg import native as N
    H, W = P.AFFINE_HW
    worst = 0.0
    for B in P.AFFINE_BATCHES:
        mb, m = _padded(6 * B, hip_device)
        ib, mi = _padded(6 * B, hip_device)
        ctr = _counter(hip_device, start)
        N.call('ssseg_affine_draw_dev', N.dev_ptr(m), N.dev_ptr(mi), B, H, W, *P.AFFINE_RANGE, seed, N.dev_ptr(ctr),
               N.stream())
        torch.cuda.synchronize()
        assert _pad_untouched(mb) and _pad_untouched(ib) and _value(ctr) == (start + B) % 2 ** 64
        theta, s, ref, ref_inv = P.affine_draw(B, H, W, *P.AFFINE_RANGE, seed, start)
        assert float(np.abs(theta).max()) <= 15 and float(s.min()) >= 0.75 and float(s.max()) <= 1.25
        worst = max(worst, P.check_affine(m.view(B, 6).cpu().numpy(), ref, H, W, f'A B={B}'),
                    P.check_affine(mi.view(B, 6).cpu().numpy(), ref_inv, H, W, f'A^-1 B={B}'))
    print(f'seed {seed:#x} counter {start:#x}: affine, largest error / bound {worst:.3f} at B {P.AFFINE_BATCHES}')


# ---- 3. ISO hue noise ------------------------------------------------------------------------------------------------
def test_iso_hue_noise(hip_device):
    """test_iso_finish's set-up (n = 3, 64 x 64) with colour std 20 and intensity 0 on sample 1: the hue noise is
    predicted on the host (u01 of c0 and c1 at counter = pixel, c2 = image, c3 = 0x150) and handed to the oracle; that
    test's tolerance.  Sample 0 (std 0) and sample 2 (ISO off) bracket it."""
    from data import device_augment as DA
    from ssseg import native as N
    rng = np.random.default_rng(9)
    n, H, W, seed = 3, 64, 64, 1234
    img = rng.integers(0, 256, size=(n, H, W, 3)).astype(np.float32)
    cps = (DA.ColorParams * n)()
    cps[0].iso = 1
    cps[1].iso, cps[1].iso_color_std, cps[1].iso_intensity = 1, 20.0, 0.0
    d_p = torch.frombuffer(bytearray(bytes(cps)), dtype=torch.uint8).to(hip_device)
    x = torch.from_numpy(img).to(hip_device)
    out = torch.empty((n, 3, H, W), device=hip_device)
    st = torch.zeros((n, 2), device=hip_device, dtype=torch.float64)
    N.call('ssseg_aug_iso_finish', N.dev_ptr(x), N.dev_ptr(out), n, H, W, N.dev_ptr(d_p), N.dev_ptr(st), seed, N.stream())
    got = out.cpu().numpy()
    ref = P.iso_reference(img, (0.0, 20.0, None), seed)
    for i in range(n):
        levels, equal = P.check_levels(got[i], ref[i], f'sample {i}')
        print(f'sample {i}: largest difference {levels:.3f} levels, {equal:.4f} of the values equal')
    # the noise is there: sample 1 is far from its noise-free conversion
    assert np.abs(got[1] - P.iso_reference(img[1:2], (0.0,), seed)[0]).max() > 20.0 / 255


# ---- 4. the production path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,ranges', P.END_TO_END)
def test_cowmix_masks_end_to_end(hip_device, shape, ranges):
    """generate_cowmix_masks_like with the device source, seed and counter set: the masks equal the oracle's
    (oracle/cowmix_ref.py fed with the host-predicted p, sigma and noise) outside the band |field - thr| < 4E + 1e-5 std,
    which may hold at most 0.2 % of the pixels; thr within 1e-5 |thr| + 2E; the counter ends at the documented advance."""
    import cowmix
    from ssseg import ops
    B, H, W = shape
    seed, start = P.SEEDS[1], 2 ** 32 - 3
    assert cowmix.NOISE_SOURCE == 'device'
    example = torch.zeros(B, 1, H, W, device=hip_device)
    key = hip_device.index if hip_device.index is not None else torch.cuda.current_device()
    old_seed, old_ctr = cowmix._DEVICE_RNG['seed'], cowmix._DEVICE_RNG['ctr'].get(key)
    try:
        cowmix._DEVICE_RNG['seed'] = seed
        ctr = cowmix._DEVICE_RNG['ctr'][key] = _counter(hip_device, start)
        mask = cowmix.generate_cowmix_masks_like(example, ranges[:2], ranges[2:])
        assert _value(ctr) == start + P.cowmix_advance(B, H * W)
        ctr.fill_(start)                                          # the same draws again, with the field and thr
        p, sig, noise = cowmix.draw_inputs(example, ranges[:2], ranges[2:])
        mask2, field, thr = ops.cowmix_mask(noise, sig, p, return_field=True)
        torch.cuda.synchronize()
        assert _value(ctr) == start + P.cowmix_advance(B, H * W)
    finally:
        cowmix._DEVICE_RNG['seed'] = old_seed
        if old_ctr is None:
            del cowmix._DEVICE_RNG['ctr'][key]
        else:
            cowmix._DEVICE_RNG['ctr'][key] = old_ctr
    assert tuple(mask.shape) == (B, 1, H, W) and mask.dtype == example.dtype and torch.equal(mask, mask2)
    ref = P.cowmix_reference(B, H, W, ranges, seed, start)
    assert ref['k_clearance'] > 1e-3, ref['k_clearance']         # the device's sigma gives the same window size K
    rp = P.check_ulp(p.cpu().numpy(), ref['p'], 'p')
    rs = P.check_sigma(sig.cpu().numpy(), ref['sigma'], ref['a'], ranges[2], ranges[3], 'sigma')
    rz = P.check_normals(noise.cpu().numpy().reshape(-1), ref['noise'], ref['rad'], 'noise')
    frac, inside, rt = P.check_masks(mask.cpu().numpy().reshape(B, H, W), thr.cpu().numpy(), ref, f'{shape} {ranges}')
    ferr = float(np.abs(field.cpu().numpy().reshape(B, H, W).astype(np.float64) - ref['field']).max())
    print(f'{shape} {ranges}: error / bound p {rp:.3f} sigma {rs:.3f} noise {rz:.3f} thr {rt:.3f}; band holds {frac:.5f} '
          f'of the pixels (cap 0.002), {inside} of them differ; field error {ferr:.3e} (E = {P.E_NORMAL:.3e}); '
          f'mask mean {float(mask.mean()):.4f}')
