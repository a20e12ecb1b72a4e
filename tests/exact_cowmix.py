"""Operands, host restatements and stage-by-stage comparison functions for the CowMix mask kernels (csrc/cowmix.hip;
test_cowmix_exact*.py).  Nothing here imports ssseg: the comparison functions take the device's result as a plain dict
of host arrays (`run`), so the host file can feed them a model's or a mutant's output instead.

ssseg_cowmix_mask leaves every intermediate where the caller can read it: K, the taps, the vertical pass and the
statistics in the workspace (carve, cowmix.hip: stats[B][2] f64, K in 16 bytes, taps[B][1023] f32, tmp[B][H][W]
f32, thr[B] f32, each aligned to 16 bytes), the field and the threshold in field_out / thr_out.  Each stage is checked
against ITS OWN inputs as the device produced them.

  stage                 tier       check
  1 K                   equal      oracle window_size (Python's round: half to even); -1 beyond KCAP
    taps                measured   4 x max(oracle fp32 taps' relative error against fp64, 2^-23) per element
                        derived    |sum - 1| <= K 2^-24; off-centre window asserted directly
  2 vertical pass tmp   bits       fma32 chain, k ascending, zero outside, the device's taps
  3 horizontal pass     bits       the same over columns, from the device's tmp
  4 stats               bounded    n 2^-53 sum|term| against a long double sum of the device's field
    thr                 bounded    1/2 ulp + (4 m + 6) 2^-24 M, m = ERFINV_M (measured); bits of float32(mean) at p = 1/2
  5 mask                bits       field > thr at every pixel, from the device's field and thr; values in {0, 1}
  6 in place            bits       field_out = NULL: the same mask
  7 end to end          as before  oracle masks outside the tie band 1e-5 std; under 1e-3 of the pixels inside it

Measured figures (printed by the checks; one MI355X, every case): the oracle's fp32 taps are within 3.6e-7 relative
of the fp64 Gaussian over the taps in fp32's normal range (worst at K = 1023; 0 at K = 1; in the multi-sigma case the
tail of the sigma = 2 sample lies below the normal range and only 51 of its 129 taps count), the device's within 3.6e-7
too; the one-ulp floor sets the taps bound at sigma = 0.5, 2, 2.5 and K = 1 (oracle error 0 to 1.1e-7), the measured
error (2.3e-7 to 3.6e-7) at the other nine (K, sigma) pairs, and check_taps prints which; ERFINV_M, the worst relative difference between scipy's erfinv rounded to fp32 and in fp64 over 4094 arguments, is
0.970 x 2^-24 (test_cowmix_exact_host.py asserts both host figures); the device's threshold is at most 2.46 x 2^-24 M
from the fp64 expression (bound 1/2 ulp + 9.88), the statistics at most 0.0022 of their bound, and the band of stage 7
holds at most 7.6e-6 of the pixels.
"""
import functools

import numpy as np
import torch

import exact_aux as A
from exact import _gen
from exact_step import fma32, same_bits
from oracle import cowmix_ref

F32 = np.float32
LD = np.longdouble
U24, U53 = 2.0 ** -24, 2.0 ** -53
KCAP, KC = 1023, 128            # cowmix.hip: KCAP, KC
VT = (64, 64)                   # vertical pass tile: rows, columns (cowmix_vblur_kernel, VTH)
HT = (8, 256)                   # horizontal pass tile (cowmix_hblur_kernel, HROWS x HTW)
SWEEP = 4096 * 256              # pixels one sweep of the threshold kernel covers
SQRT2_F = F32(1.41421354)       # cowmix_finalize_kernel
FLT_MIN = 2.0 ** -126
TAPS_MARGIN, ERFINV_MARGIN = 4.0, 4.0
P_CYCLE = (0.5, 0.3, 0.7)

# name, (B, H, W), sigmas
CASES = (
    ('k1', (2, 9, 13), (0.16, 0.16)),
    ('k1-second-sweep', (1, 1025, 1025), (0.16,)),
    ('half-0.5', (3, 20, 20), (0.5, 0.5, 0.5)),
    ('half-1.5', (3, 20, 20), (1.5, 1.5, 1.5)),
    ('half-2.5', (3, 20, 20), (2.5, 2.5, 2.5)),
    ('k127', (1, 70, 300), (21.0,)),
    ('k129', (1, 70, 300), (21.3,)),
    ('k257', (1, 70, 300), (42.67,)),
    ('multi-sigma', (3, 65, 257), (2.0, 21.3, 8.0)),
    ('ragged-63x255', (2, 63, 255), (6.0, 6.0)),
    ('ragged-7x261', (2, 7, 261), (6.0, 6.0)),
    ('ragged-129x3', (2, 129, 3), (6.0, 6.0)),
    ('kcap', (1, 40, 300), (170.3,)),
)
EXPECT_K = {'k1': 1, 'k1-second-sweep': 1, 'half-0.5': 5, 'half-1.5': 9, 'half-2.5': 17, 'k127': 127, 'k129': 129,
            'k257': 257, 'multi-sigma': 129, 'ragged-63x255': 37, 'ragged-7x261': 37, 'ragged-129x3': 37, 'kcap': 1023}
BEYOND = ('beyond-kcap', (1, 16, 16), (170.7,))
IMPULSE = ('impulse', (1, 130, 260), (3.0,))
IMPULSE_AT = ((0, 0), (129, 259), (63, 255), (64, 256), (7, 127), (8, 128))
DESIGNED = ('designed-stats', (2, 9, 13), (0.16, 0.16))
CASE_BY_NAME = {c[0]: c for c in CASES + (BEYOND, IMPULSE, DESIGNED)}


def _a16(x):
    return (x + 15) & ~15


def carve(B, H, W):
    """carve (cowmix.hip): name -> (byte offset, dtype, shape), and the total"""
    out, off = {}, 0
    out['stats'] = (off, np.float64, (B, 2))
    off = _a16(off + 8 * 2 * B)
    out['K'] = (off, np.int32, (1,))
    off = _a16(off + 16)
    out['taps'] = (off, F32, (B, KCAP))
    off = _a16(off + 4 * KCAP * B)
    out['tmp'] = (off, F32, (B, H, W))
    off = _a16(off + 4 * B * H * W)
    out['thr_ws'] = (off, F32, (B,))
    off = _a16(off + 4 * B)
    return out, off


def decode(ws_bytes, B, H, W, expect_total):
    lay, total = carve(B, H, W)
    assert total == expect_total, f'workspace layout changed: restated {total} bytes, library says {expect_total}'
    assert ws_bytes.dtype == np.uint8 and ws_bytes.size >= total
    out = {}
    for name, (o, dt, shape) in lay.items():
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = ws_bytes[o:o + n].view(dt).reshape(shape).copy()
    out['K'] = int(out['K'][0])
    return out


def tiles(H, W):
    """(vertical tiles y, x), (horizontal tiles y, x)"""
    return (-(-H // VT[0]), -(-W // VT[1])), (-(-H // HT[0]), -(-W // HT[1]))


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def sigmas_of(case):
    return np.asarray(case[2], F32)


def p_of(case):
    B = case[1][0]
    return np.asarray([P_CYCLE[b % 3] for b in range(B)], F32)


@functools.lru_cache(maxsize=None)
def noise_of(name, variant=None):
    """fp32 [B, H, W], read-only.  Standard normals; 'impulse' with variant (y, x): zeros and one 1.0;
    'designed-stats': integers -3 .. 3 (variant 'tie': adjusted to sum exactly 0 per sample)."""
    _, (B, H, W), _ = CASE_BY_NAME[name]
    g = _gen('cowmix', name)
    if name == 'impulse':
        n = np.zeros((B, H, W), F32)
        n[0, variant[0], variant[1]] = 1.0
    elif name == 'designed-stats':
        n = torch.randint(-3, 4, (B, H, W), generator=g).float().numpy()
        if variant == 'tie':
            for b in range(B):
                flat = n[b].reshape(-1)
                i = 0
                while flat.sum() != 0:
                    step = -np.sign(flat.sum())
                    if abs(flat[i] + step) <= 3:
                        flat[i] += step
                    i += 1
    else:
        n = torch.randn(B, H, W, generator=g, dtype=torch.float32).numpy().copy()
    n.setflags(write=False)
    return n


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: K and the taps
# ---------------------------------------------------------------------------------------------------------------------
def window_half_up(sigmas):
    """the mutation: round half up"""
    return int(np.floor(float(np.max(sigmas)) * 3 + 0.5)) * 2 + 1


def window_half_down(sigmas):
    """the other mutation: round half down (and what truncating the half away would give)"""
    return int(np.ceil(float(np.max(sigmas)) * 3 - 0.5)) * 2 + 1


def taps64(K, sigma):
    """the reference's off-centre grid x = k + floor(-K / 2) (K is odd: no half step), exp(-x^2 / (2 sigma^2))
    normalised, in fp64 from the fp32 sigma"""
    x = np.arange(K, dtype=np.float64) + (-K) // 2
    s = float(F32(sigma))
    g = np.exp(-(x * x) / (2.0 * s * s))
    return g / g.sum()


def taps_centred(K, sigma):
    """the mutation: a symmetric grid x = k - K // 2, fp32 like the oracle"""
    x = np.arange(K, dtype=F32) - F32(K // 2)
    s = F32(sigma)
    g = np.exp(-(x * x) / F32(float(F32(2) * s * s))).astype(F32)
    return (g / g.sum(dtype=F32)).astype(F32)


def check_taps(run, sigmas, what):
    """K equals the oracle's window_size (-1 beyond KCAP, and nothing else is checked then).  taps[b][0:K] per element:
    |got - g64| <= 4 E g64 + 2^-126 with E = max(the oracle's own fp32 taps' worst relative error against g64 over
    the taps in fp32's normal range, 2^-23).  The oracle and the kernel form the same fp32 argument -(x x) / (2 s s)
    (its rounding, times the argument, is the bulk of E at large arguments and common to both); they differ in expf
    (numpy's against the device's), the order of the normalising sum and nothing else, which 4 x allows for.  The floor
    of one fp32 ulp keeps the bound from collapsing where the oracle happens to be exact (K = 1: g = 1) or nearly so
    on a handful of taps.  Below the smallest normal number (the tail of a small sigma in a window sized by a large
    one) only the absolute term holds: an expf may flush there.
    Each sample's taps sum to 1 within K 2^-24.  The window is off-centre: the peak is tap (K + 1) / 2, and
    taps[k] != taps[K - 1 - k] wherever both are in the normal range."""
    sig = np.asarray(sigmas, F32)
    K = cowmix_ref.window_size(sig)
    want = K if K <= KCAP else -1
    print(f'{what}: K device {run["K"]} oracle {K}')
    assert run['K'] == want, f'{what}: K {run["K"]} != {want}'
    if want < 0:
        return None
    worst_or, worst_dev = 0.0, 0.0
    for b, s in enumerate(sig):
        g64 = taps64(K, s)
        g32 = cowmix_ref.gaussian_taps(K, s).astype(np.float64)
        got = run['taps'][b, :K].astype(np.float64)
        normal = g64 >= 4 * FLT_MIN
        e_or = float((np.abs(g32 - g64)[normal] / g64[normal]).max())
        e_dev = float((np.abs(got - g64)[normal] / g64[normal]).max())
        worst_or, worst_dev = max(worst_or, e_or), max(worst_dev, e_dev)
        scale = max(e_or, 2.0 ** -23)
        bound = TAPS_MARGIN * scale * g64 + FLT_MIN
        bad = ~(np.abs(got - g64) <= bound)
        print(f'{what}: taps sample {b} sigma {float(s)!r}: oracle fp32 error {e_or:.3e} device {e_dev:.3e} (relative, '
              f'{int(normal.sum())} of {K} taps normal); bound {TAPS_MARGIN:g} x {scale:.3e} set by '
              f'{"the measured oracle error" if e_or >= 2.0 ** -23 else "the one-ulp floor 2^-23"}; '
              f'sum - 1 = {got.sum() - 1:.3e} (bound {K * U24:.3e})')
        assert not bad.any(), f'{what}: sample {b}: {int(bad.sum())} taps outside 4 x the oracle\'s error, first {np.argwhere(bad)[0]}'
        assert abs(got.sum() - 1.0) <= K * U24, f'{what}: sample {b}: taps sum to {got.sum()!r}'
        if K >= 3:
            assert int(np.argmax(got)) == (K + 1) // 2, f'{what}: sample {b}: peak at tap {int(np.argmax(got))}'
            k = np.arange(K // 2)
            both = normal[k] & normal[K - 1 - k]
            assert both.any() and (got[k][both] != got[K - 1 - k][both]).all(), f'{what}: sample {b}: symmetric taps'
        else:
            assert got[0] == 1.0, f'{what}: the single tap is {got[0]!r}'
    return worst_or, worst_dev


# ---------------------------------------------------------------------------------------------------------------------
# stages 2, 3: the two passes
# ---------------------------------------------------------------------------------------------------------------------
def blur_restate(src, taps, K, axis, descending=False):
    """out = sum_k g[k] * in[. - K // 2 + k] along `axis` (1: rows, 2: columns) as the kernels form it
    (the tap loops of cowmix_vblur_kernel and cowmix_hblur_kernel): acc = fmaf(g[k], in, acc), k ascending from acc = 0,
    zero outside the image,
    per-sample taps [B, >= K]"""
    src = np.asarray(src, F32)
    B, H, W = src.shape
    pad = K // 2
    shape = (B, H + 2 * pad, W) if axis == 1 else (B, H, W + 2 * pad)
    buf = np.zeros(shape, F32)
    if axis == 1:
        buf[:, pad:pad + H] = src
    else:
        buf[:, :, pad:pad + W] = src
    acc = np.zeros((B, H, W), F32)
    for k in (range(K - 1, -1, -1) if descending else range(K)):
        sl = buf[:, k:k + H] if axis == 1 else buf[:, :, k:k + W]
        acc = fma32(taps[:, k].reshape(B, 1, 1), sl, acc)
    return acc


def check_blur(run, noise, what):
    K = run['K']
    same_bits(run['tmp'], blur_restate(noise, run['taps'], K, 1), f'{what}: vertical pass')
    same_bits(run['field'], blur_restate(run['tmp'], run['taps'], K, 2), f'{what}: horizontal pass')
    print(f'{what}: both passes bit-equal to the fma32 chain over {K} taps; tiles (v, h) {tiles(*noise.shape[1:])}')


def check_impulse(run, at, what):
    """one 1.0 at (y0, x0): the vertical pass leaves g[ky] in column x0 at y = y0 + K // 2 - ky, the horizontal pass
    fl32(g[kx] g[ky]) at x = x0 + K // 2 - kx; everything else is exactly +0"""
    K, pad = run['K'], run['K'] // 2
    g = run['taps'][0, :K]
    B, H, W = run['field'].shape
    want = np.zeros((H, W), F32)
    ys, xs = at[0] + pad - np.arange(K), at[1] + pad - np.arange(K)
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    want[np.ix_(ys[oky], xs[okx])] = g[oky][:, None] * g[okx][None, :]
    same_bits(run['field'][0], want, f'{what}: impulse response')
    print(f'{what}: {int(oky.sum())} x {int(okx.sum())} of the {K} x {K} support inside the image, bit-equal; '
          f'{int((want == 0).sum())} pixels exactly 0')


# ---------------------------------------------------------------------------------------------------------------------
# stage 4: statistics and threshold
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def erfinv_m():
    """the worst relative difference, in units of 2^-24, between scipy's erfinv rounded to fp32 and in fp64, over the
    4095 arguments j / 2048 - 1: what a correctly rounded erfinvf would show.  The device's erfinvf gets 4 x that."""
    from scipy.special import erfinv
    a = (np.arange(1, 4096) / 2048.0 - 1.0)
    a = a[a != 0]
    v = erfinv(a)
    return float((np.abs(v.astype(F32).astype(np.float64) - v) / np.abs(v)).max() / U24)


def thr_restate(stats, p, n, biased=False):
    """cowmix_finalize_kernel (cowmix.hip) on the host in the kernel's precisions, erfinvf taken as scipy's
    erfinv rounded to fp32 (a model for the host file; the GPU comparison uses thr_reference)"""
    from scipy.special import erfinv
    s1, s2 = stats[:, 0], stats[:, 1]
    mean = s1 / n
    var = np.maximum((s2 - s1 * mean) / (n if biased else n - 1.0), 0.0)
    a = F32(2) * np.asarray(p, F32) - F32(1)
    with np.errstate(all='ignore'):
        factor = erfinv(a.astype(np.float64)).astype(F32) * SQRT2_F
        return (factor * np.sqrt(var).astype(F32) + mean.astype(F32)).astype(F32)


def thr_reference(stats, p, n):
    """(thr in fp64, M = |factor| std + |mean|, float32(mean)) from the device's stats; the fp32 argument 2 p - 1 is
    exact in the kernel's form (2 p is exact, one rounding with or without a contraction)"""
    from scipy.special import erfinv
    s1, s2 = stats[:, 0], stats[:, 1]
    mean = s1 / n
    std = np.sqrt(np.maximum((s2 - s1 * mean) / (n - 1.0), 0.0))
    a = (F32(2) * np.asarray(p, F32) - F32(1)).astype(np.float64)
    with np.errstate(all='ignore'):
        factor = erfinv(a) * float(SQRT2_F)
        return factor * std + mean, np.abs(factor) * std + np.abs(mean), mean.astype(F32)


def check_stats(run, p, what):
    """stats[b] = (sum f, sum f^2) of the device's field against long double sums (each square is exact in fp64): the
    order of the atomic adds is free, so |got - ref| <= n 2^-53 sum|term|, n = H W.
    thr[b] against thr_reference from the device's stats: 1/2 ulp32 + (4 m + 6) 2^-24 M with m = ERFINV_M -- erfinvf
    held to 4 x the rounding of a correctly rounded one --, and 6 for: the product with sqrt(2)'s fp32 value (1), the
    fp32 roundings of std and mean (2), the product and the sum or their fma (2), and the fp64 variance (1, far less).
    An infinite factor (p = 0 or 1) must give the same infinity; p = 1/2 (factor 0) the bits of float32(mean).
    The workspace's thr and thr_out hold the same bits."""
    f = run['field'].astype(np.float64)
    B = f.shape[0]
    n = f.shape[1] * f.shape[2]
    worst = 0.0
    for b in range(B):
        for j, term in enumerate((f[b], f[b] * f[b])):
            ref, mag = term.astype(LD).sum(), np.abs(term).astype(LD).sum()
            err, bound = abs(LD(run['stats'][b, j]) - ref), n * U53 * mag
            worst = max(worst, float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, f'{what}: stats[{b}][{j}] {run["stats"][b, j]!r} vs {float(ref)!r} (bound {float(bound):.3e})'
    same_bits(run['thr_ws'], run['thr'], f'{what}: thr_out against the workspace thr')
    ref, M, meanf = thr_reference(run['stats'], p, n)
    m = erfinv_m()
    k = ERFINV_MARGIN * m + 6
    with np.errstate(all='ignore'):
        units = np.abs(run['thr'].astype(np.float64) - ref) / (U24 * M)
    print(f'{what}: stats worst error {worst:.4f} of n 2^-53 sum|term|; thr {run["thr"]} reference {ref}, error '
          f'{units} x 2^-24 M (bound 1/2 ulp + {k:.2f}), erfinv rounding m = {m:.3f}')
    for b in range(B):
        if float(p[b]) == 0.5:
            same_bits(run['thr'][b:b + 1], meanf[b:b + 1], f'{what}: thr[{b}] at p = 1/2')
        elif not np.isfinite(ref[b]):
            assert run['thr'][b] == ref[b], f'{what}: thr[{b}] {run["thr"][b]!r} vs {ref[b]!r}'
        else:
            A.assert_bounded(torch.from_numpy(run['thr'][b:b + 1]), torch.from_numpy(ref[b:b + 1]),
                             torch.from_numpy(M[b:b + 1]), k, 'f32', f'{what}: thr[{b}]')


# ---------------------------------------------------------------------------------------------------------------------
# stages 5-7
# ---------------------------------------------------------------------------------------------------------------------
def check_mask(run, what):
    """mask = field > thr ? 1 : 0, bit for bit at every pixel, from the device's own field and threshold: no tie band,
    no exempt pixel"""
    want = (run['field'] > run['thr'].reshape(-1, 1, 1)).astype(F32)
    same_bits(run['mask'], want, f'{what}: mask')
    assert np.isin(run['mask'], (0.0, 1.0)).all()
    print(f'{what}: mask bit-equal to field > thr at {want.size} pixels, {float(want.mean()):.4f} ones')


def check_in_place(run, mask_in_place, what):
    same_bits(mask_in_place, run['mask'], f'{what}: in-place path (field_out = NULL)')


@functools.lru_cache(maxsize=None)
def oracle(name, variant=None, p=None):
    case = CASE_BY_NAME[name]
    pp = p_of(case) if p is None else np.asarray(p, F32)
    return cowmix_ref.cowmix_masks(np.array(noise_of(name, variant)), sigmas_of(case), pp)


def band_share(field, thr, std):
    return float((np.abs(field - thr.reshape(-1, 1, 1)) < 1e-5 * std.reshape(-1, 1, 1)).mean())


def check_end_to_end(run, name, what, variant=None, p=None):
    """against oracle/cowmix_ref.py under the bounds of test_hip_losses.py::test_cowmix_mask_bit_exact_outside_tie_band
    (thr rtol 1e-5 atol 1e-6, field atol 2e-6, masks equal outside the band |field - thr| < 1e-5 std), and the band
    holds under 1e-3 of the pixels"""
    mask, field, thr, mean, std = oracle(name, variant, None if p is None else tuple(float(v) for v in p))
    share = band_share(run['field'], thr, std)
    diff = run['mask'] != mask
    band = np.abs(run['field'] - thr.reshape(-1, 1, 1)) < 1e-5 * std.reshape(-1, 1, 1)
    print(f'{what}: end to end: thr {run["thr"]} oracle {thr}; field max error '
          f'{float(np.abs(run["field"] - field).max()):.3e}; {int(diff.sum())} mask pixels differ, '
          f'{int((diff & ~band).sum())} outside the band; share of pixels in the band {share:.2e}')
    np.testing.assert_allclose(run['thr'], thr, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(run['field'], field, rtol=0, atol=2e-6)
    assert not (diff & ~band).any()
    assert share < 1e-3


def check_all(run, name, what, variant=None, p=None, mask_in_place=None, end_to_end=True):
    """every stage in order (end_to_end=False leaves stage 7 out: the 'tie' inputs sit in its band by design)"""
    case = CASE_BY_NAME[name]
    noise, sig = noise_of(name, variant), sigmas_of(case)
    p = p_of(case) if p is None else np.asarray(p, F32)
    fig = check_taps(run, sig, what)
    check_blur(run, noise, what)
    check_stats(run, p, what)
    check_mask(run, what)
    if mask_in_place is not None:
        check_in_place(run, mask_in_place, what)
    if end_to_end:
        check_end_to_end(run, name, what, variant, p)
    return fig


def check_beyond_kcap(run, rc, what):
    """K > KCAP: the documented result is a NaN mask and threshold and a return code of 0"""
    assert rc == 0 and run['K'] == -1, (rc, run['K'])
    assert np.isnan(run['mask']).all() and np.isnan(run['thr']).all() and np.isnan(run['thr_ws']).all(), \
        f'{what}: mask / thr not all NaN'


# ---------------------------------------------------------------------------------------------------------------------
# a host model of the device
# ---------------------------------------------------------------------------------------------------------------------
def device_model(noise, sigmas, p, mutate=None):
    """What a device that follows cowmix.hip returns (numpy's expf and scipy's erfinv in place of the device's), or one
    that carries a named fault: 'centred' (a symmetric tap grid), 'half-up' (K rounded half up), 'taps0' (sample 0's
    taps used for every sample), 'descending' (tap order K - 1 .. 0), 'biased' (variance / n), 'ge' (mask = field >=
    thr)."""
    noise, sig, p = np.asarray(noise, F32), np.asarray(sigmas, F32), np.asarray(p, F32)
    B, H, W = noise.shape
    K = window_half_up(sig) if mutate == 'half-up' else cowmix_ref.window_size(sig)
    run = {'K': K if K <= KCAP else -1, 'taps': np.full((B, KCAP), np.nan, F32)}
    if run['K'] < 0:
        nan = np.full((B, H, W), np.nan, F32)
        run.update(tmp=nan, field=nan, mask=nan.copy(), thr=np.full(B, np.nan, F32), thr_ws=np.full(B, np.nan, F32),
                   stats=np.zeros((B, 2)))
        return run
    for b in range(B):
        run['taps'][b, :K] = taps_centred(K, sig[b]) if mutate == 'centred' else cowmix_ref.gaussian_taps(K, sig[b])
    used = np.repeat(run['taps'][:1], B, 0) if mutate == 'taps0' else run['taps']
    run['tmp'] = blur_restate(noise, used, K, 1, mutate == 'descending')
    run['field'] = blur_restate(run['tmp'], used, K, 2, mutate == 'descending')
    f = run['field'].astype(np.float64).reshape(B, -1)
    run['stats'] = np.stack([f.sum(1), (f * f).sum(1)], 1)
    run['thr'] = thr_restate(run['stats'], p, float(H * W), biased=mutate == 'biased')
    run['thr_ws'] = run['thr'].copy()
    t = run['thr'].reshape(B, 1, 1)
    run['mask'] = ((run['field'] >= t) if mutate == 'ge' else (run['field'] > t)).astype(F32)
    return run
