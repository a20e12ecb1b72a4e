"""The CowMix mask kernels (csrc/cowmix.hip), stage by stage, against the host restatements of tests/exact_cowmix.py.

ssseg_cowmix_mask is called through ssseg.native with field_out and thr_out set, on the test's own workspace, prefilled
(like every output) with 0xFF bytes / NaN so that an element a kernel leaves unwritten cannot pass.  The workspace is
decoded by the restated layout -- whose total must equal ssseg_cowmix_workspace_bytes -- and every stage is compared
with ITS OWN inputs as the device produced them (exact_cowmix.check_all): K equal, the taps to 4 x the oracle's own fp32
error, both passes bit for bit against the fma32 chain, the statistics against long double sums, the threshold per
element, and the mask bit for bit at every pixel -- no tie band, no exempt pixel.  The cases of exact_cowmix.CASES are
the smallest at which one edge of the kernels is live (test_cowmix_exact_host.py asserts the edge).  Every test prints
its figures before it asserts."""
import numpy as np
import pytest
import torch

import exact_cowmix as C
from exact_step import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32


def _run(dev, noise, sigmas, p, with_field=True):
    """one call of ssseg_cowmix_mask: the decoded workspace, mask, field and thr (None without field_out), the return
    code"""
    from ssseg import native as N
    B, H, W = noise.shape
    nb = int(N.lib().ssseg_cowmix_workspace_bytes(B, H, W))
    nd = torch.from_numpy(np.array(noise, F32)).to(dev)
    sd = torch.from_numpy(np.asarray(sigmas, F32).copy()).to(dev)
    pd = torch.from_numpy(np.asarray(p, F32).copy()).to(dev)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    mask = torch.full((B, H, W), float('nan'), device=dev)
    field = torch.full((B, H, W), float('nan'), device=dev) if with_field else None
    thr = torch.full((B,), float('nan'), device=dev) if with_field else None
    rc = N.lib().ssseg_cowmix_mask(nd.data_ptr(), sd.data_ptr(), pd.data_ptr(), B, H, W, mask.data_ptr(),
                                   field.data_ptr() if with_field else None, thr.data_ptr() if with_field else None,
                                   ws.data_ptr(), nb, N.stream())
    torch.cuda.synchronize()
    run = C.decode(ws.cpu().numpy(), B, H, W, nb)
    run.update(mask=mask.cpu().numpy(), field=field.cpu().numpy() if with_field else None,
               thr=thr.cpu().numpy() if with_field else None)
    return run, rc


def _both(dev, name, variant=None, p=None):
    case = C.CASE_BY_NAME[name]
    noise, sig = C.noise_of(name, variant), C.sigmas_of(case)
    p = C.p_of(case) if p is None else np.asarray(p, F32)
    run, rc = _run(dev, noise, sig, p)
    inplace, rc2 = _run(dev, noise, sig, p, with_field=False)
    assert rc == 0 and rc2 == 0
    return run, inplace['mask']


@pytest.mark.parametrize('name', [c[0] for c in C.CASES])
def test_cowmix_stages(hip_device, name):
    """Stages 1-7 of exact_cowmix at one edge case each; with K = 1 the single tap is 1.0 and the field is the noise"""
    run, inplace = _both(hip_device, name)
    assert run['K'] == C.EXPECT_K[name]
    C.check_all(run, name, name, mask_in_place=inplace)
    if run['K'] == 1:
        same_bits(run['field'], np.array(C.noise_of(name)), f'{name}: field at K = 1')


def test_cowmix_beyond_kcap(hip_device):
    """K = 1025 > KCAP: the documented result -- mask and thr all NaN, return code 0 -- with and without field_out;
    the kernels return early and the field is never written"""
    name, shape, sig = C.BEYOND
    noise, p = C.noise_of(name), np.asarray([0.5], F32)
    run, rc = _run(hip_device, noise, np.asarray(sig, F32), p)
    print(f'{name}: rc {rc} K {run["K"]} thr {run["thr"]} mask NaN share {float(np.isnan(run["mask"]).mean())}')
    C.check_taps(run, np.asarray(sig, F32), name)
    C.check_beyond_kcap(run, rc, name)
    assert np.isnan(run['field']).all() and np.isnan(run['tmp']).all()
    inplace, rc = _run(hip_device, noise, np.asarray(sig, F32), p, with_field=False)
    assert rc == 0 and inplace['K'] == -1 and np.isnan(inplace['mask']).all()


@pytest.mark.parametrize('at', C.IMPULSE_AT, ids=[f'{y}-{x}' for y, x in C.IMPULSE_AT])
def test_cowmix_impulse(hip_device, at):
    """one 1.0 in a field of zeros, at the image corners and on both sides of the 64-row / 256-column (vertical pass)
    and 8-row / 128-column (horizontal pass: a thread's second run of columns) edges: the field is fl32(g[ky] g[kx]) on
    the K x K support, shifted by the off-centre window, and exactly 0 elsewhere"""
    what = f'impulse {at}'
    run, inplace = _both(hip_device, 'impulse', at)
    C.check_impulse(run, at, what)
    C.check_all(run, 'impulse', what, variant=at, mask_in_place=inplace)


def test_cowmix_designed_statistics(hip_device):
    """integers -3 .. 3 through a K = 1 window: the field is the noise and both sums are exact, so stats are the BITS of
    the integer sums; at p = 1/2 and 0.3 no value lies within 1e-3 of the threshold, so the mask is exact at every
    pixel against the fp64 threshold; p = 0 gives all ones, p = 1 all zeros; and zeros sitting ON the threshold (the
    'tie' variant: sum 0, p = 1/2, thr = 0.0) are not in the mask"""
    n = np.array(C.noise_of('designed-stats'))
    B = n.shape[0]
    flat = n.reshape(B, -1).astype(np.int64)
    sums = np.stack([flat.sum(1), (flat ** 2).sum(1)], 1).astype(np.float64)
    for p in ((0.5, 0.3), (0.3, 0.5)):
        p = np.asarray(p, F32)
        run, inplace = _both(hip_device, 'designed-stats', p=p)
        print(f'designed p {p}: stats {run["stats"].tolist()} integer sums {sums.tolist()} thr {run["thr"]}')
        same_bits(run['field'], n, 'designed: field')
        same_bits(run['stats'], sums, 'designed: stats')
        ref, _, _ = C.thr_reference(sums, p, float(n[0].size))
        same_bits(run['mask'], (n > ref.reshape(B, 1, 1)).astype(F32), 'designed: mask against the fp64 threshold')
        C.check_all(run, 'designed-stats', f'designed p {p}', p=p, mask_in_place=inplace)
    run, inplace = _both(hip_device, 'designed-stats', p=(0.0, 1.0))
    print(f'designed p (0, 1): thr {run["thr"]}')
    assert run['thr'][0] == -np.inf and run['thr'][1] == np.inf
    same_bits(run['mask'], np.stack([np.ones_like(n[0]), np.zeros_like(n[1])]), 'designed: p = 0 and p = 1')
    same_bits(inplace, run['mask'], 'designed: p = 0 and p = 1 in place')
    C.check_stats(run, np.asarray([0.0, 1.0], F32), 'designed p (0, 1)')
    t = np.array(C.noise_of('designed-stats', 'tie'))
    run, inplace = _both(hip_device, 'designed-stats', 'tie', p=(0.5, 0.5))
    print(f'designed tie: stats {run["stats"].tolist()} thr {run["thr"]}')
    same_bits(run['thr'], np.zeros(B, F32), 'tie: thr')
    same_bits(run['mask'], (t > 0).astype(F32), 'tie: mask')
    C.check_all(run, 'designed-stats', 'designed tie', variant='tie', p=(0.5, 0.5), mask_in_place=inplace,
                end_to_end=False)
