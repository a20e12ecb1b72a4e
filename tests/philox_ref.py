"""Host restatement (numpy) of every device-side random draw, for tests/test_device_rng.py and
tests/test_device_rng_host.py.

The one device Philox-4x32-10 (philox4x32_10 in csrc/philox.h, compiled into cowmix.hip, warp.hip, mixmask.hip, pool.hip
and augment.hip) is the standard generator (the published known-answer vectors, tests/test_device_rng_host.py): counter
(c0, c1, c2, c3) = (ctr mod 2^32, ctr >> 32, word2, word3) with ctr taken mod 2^64, key (seed mod 2^32, seed >> 32),
ten rounds, the key bumped by (0x9E3779B9, 0xBB67AE85) after each.  `philox` is that function, vectorised over the
counters; one function per consumer restates the layout (which counter and which word feeds which output) and the fp32
arithmetic as the kernel writes it.

    consumer                      counter                 word2    word3   words used
    CowMix noise (normal_kernel)  offset + B + q          0        0       (c0, c1) -> z[4q], z[4q+1]; (c2, c3) -> the next two
    CowMix p / sigma              offset + b              1        0       c0 -> p, c1 -> sigma
    affine views                  offset + b              2        0       c0 -> theta, c1 -> s
    ClassMix keys                 offset + b Q + j        3        0       c0..c3 -> classes 4 j .. 4 j + 3   (Q = ceil(C/4))
    CutMix params                 offset + B Q + b        4        0       c0..c3 -> p', u, v1, v2
    dropout                       offset + q              0x5eed   0       c0..c3 -> elements 4 q .. 4 q + 3
    ElasticTransform field        i                       0xe1a5   0       c0
    ISO noise                     pixel i                 image n  0x150   c0, c1 -> hue normal; c2 -> Poisson uniform
The first five share one per-device seed and counter (cowmix._DEVICE_RNG); dropout has a seed and a counter of its own
(ssseg.nn._DROP); the two augment draws take a fresh 64-bit seed per call and count from 0.

Advances of the shared counter per call: CowMix B + ceil(B HW / 4) + 1, affine B, mixmask B (Q + 1) whichever of the two
outputs is asked for.

The keyword arguments `rounds`, `carry`, `word2` (`noise_word2`, `params_word2`, `word3`) and `swap` exist for the
mutation tests alone (nine rounds, c1 forced to 0, another stream word, sin and cos exchanged): the comparators below
must reject a reference built with them.


Tolerances
==========
u = 2^-24 is the unit roundoff of fp32 (half an ulp relative), so a result of magnitude v that is `k ulp` off is off by
at most 2 k u |v|.  ROCm's headers only forward logf, expf, sqrtf, sincosf and cosf to the device library and state no
accuracy, so the figure used here is the one HIP's published math-API tables stay within for these five functions:
at most 2 ulp each.  No number below is fitted to an output of the device.

Exact (integer) checks -- no tolerance:
  * keys = c & 0x7fffffff; params, dropout's u and CowMix's p' = float(c >> 8) 2^-24: c >> 8 < 2^24 converts exactly
    and the power-of-two scale is exact.
  * p with the proportion range (0, 1): lo + u1 (hi - lo) = 0 + u1 * 1, exact as a product and a sum or as one FMA.
  * dropout keeps where u >= p with p rounded to fp32 (it is passed as a float); a kept 1 becomes the fp32 quotient
    1 / (1 - p) rounded to the tensor's type.
  * the uniform field 2 u01 - 1 with u01 = (k + 1) 2^-24, k = c >> 8: k + 1 <= 2^24 is exact in fp32; 2 u01 - 1 =
    (2 (k + 1) - 2^24) 2^-24 has an integer of magnitude <= 2^24 as its significand, so it is exact as a product and a
    difference, and a contracted FMA returns the same number.
  * affine theta = max_angle (2 u1 - 1): 2 u1 - 1 is exact as above, one rounded product follows.  s = lo + u2 (hi - lo)
    clamped to [lo, hi]: warp.hip is built without contraction, so it is a rounded difference, product and sum, which
    np.float32 arithmetic repeats bit for bit.

Normals (Box-Muller): z = rad * cos(ang) or rad * sin(ang), rad = sqrtf(-2 logf(u1)), ang = 6.2831855f * u2.
  u1 = (float(k) + 0.5f) 2^-24 and ang are single fp32 roundings that numpy repeats exactly (k + 0.5 rounds to even
  for k >= 2^23; for k = 2^24 - 1 it rounds to 2^24, so u1 = 1, rad = 0 and both normals are exactly 0).  The smallest u1
  is 2^-25: rad <= sqrt(2 ln 2^25) = 5.8870..., hence |z| <= 5.89.  The reference evaluates log, sqrt, cos and sin in
  fp64 from those fp32 inputs.
    logf 2 ulp: relative 4u; times -2 exact; the square root halves it to 2u; sqrtf's own 2 ulp add 4u: rad is within
    6u relative.  cos / sin: 2 ulp of a value of magnitude <= 1, where an ulp is at most 2u: absolute 4u.  The
    product rounds once more: relative u.
    |z_dev - z_ref| <= |z| (6u + u) + rad 4u + second order  <=  8u (|z_ref| + rad_ref)  =  2^-21 (|z_ref| + rad_ref).
  With |z|, rad <= 5.89 that is at most E = 2^-21 * 11.78 = 5.62e-6 anywhere.

CowMix p for a general range: p = lo + u1 (hi - lo) in fp32, hi - lo one rounded difference (repeated exactly).  As an
  FMA it is the fp64 value rounded once (1/2 ulp); uncontracted, the product rounds (<= 1/2 ulp of a number <= p,
  because lo >= 0) and the sum rounds (1/2 ulp of p): within 1 fp32 ulp of the fp64 value either way.

sigma = expf(a), a = llo + u2 (lhi - llo), llo = (float)log(sigma_lo) (fp64 log, one rounding; repeated exactly), for
  ranges with sigma_lo >= 1 (llo >= 0, so the product u2 (lhi - llo) <= a).  The device's a is off the fp64 a by at most
  u |product| + u |a| <= 2u |a| (less as an FMA); exp turns an absolute error of its argument into the same relative
  error of its value; expf's own 2 ulp add 4u:  relative error <= u (4 + 2 |a|), and the stated bound is twice that,
  2^-23 (4 + 2 |a|).  The range check sigma_lo (1 - 2^-20) <= sigma <= sigma_hi (1 + 2^-20) follows: a lies in
  [llo, lhi] up to one rounding, |a| <= ln 45 < 4 in the suite, so sigma leaves the range by less than 2^-23 * 12 < 2^-20
  relative (plus the 2^-24 of rounding log sigma_lo and log sigma_hi to fp32).

Affine matrices: the kernel builds A(theta, s) and A(-theta, 1/s) in fp64 from the fp32 theta and s and rounds every
  entry once; its fp64 cos / sin / division differ from the host's by a few fp64 ulps (2^-50 relative), which can move
  an fp32 rounding by one ulp only at a tie.  Rotation and scale entries (al, be, -be, al): within 1 fp32 ulp of
  geo_ref.mats64.  Translation entries t = cx - al cx - be cy: |theta| <= 15 degrees and 0.75 <= s <= 1.25 give
  |1 - al| <= 0.34 and |be| <= 0.35 for A and for its inverse, so |t| <= 0.69 max(cx, cy) and one fp32 rounding of it
  is at most u 0.69 max(cx, cy) -- inside the stated 2^-23 max(1, cx, cy) = 2u max(1, cx, cy).

ISO hue noise: rad * cosf(6.2831853f * u2) * std in fp32 against the same expression in fp64 differs by less than 1e-4
  degrees at std = 20 (the bound on the normals times 20); the test's tolerance is the existing one of test_iso_finish
  (one 8-bit level, more than half the values equal), against which a wrong stream is off by tens of levels.

End to end: the blurred field is a convex combination of the noise in each pass (non-negative taps that sum to 1), so
  it inherits at most E from the normals; pixels with |field_ref - thr_ref| < 4E + 1e-5 std are left out of the mask
  comparison (the band also covers the shift of the threshold: |erfinv(2p - 1) sqrt 2| <= 0.53 for p in [0.3, 0.7]),
  and the band may hold at most 0.2 % of the pixels.
"""
import math

import numpy as np

import geo_ref

MASK32 = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TWO_M24 = np.float32(1.0 / 16777216.0)
E_NORMAL = 2.0 ** -21 * 11.78

# the stream words of the consumers that share CowMix's per-device seed and counter
STREAM_NOISE, STREAM_PSIGMA, STREAM_AFFINE, STREAM_KEYS, STREAM_PARAMS = 0, 1, 2, 3, 4
STREAM_DROPOUT, STREAM_FIELD, WORD3_ISO = 0x5eed, 0xe1a5, 0x150

# the seeds and counter values of the suite: a zero key, both key halves non-zero, the largest seed the package draws
SEEDS = (0, 0x0123456789ABCDEF, 2 ** 62 - 1)
# host-offset entry points: the carry into c1 falls inside a call of more than three counters at 2^32 - 3; 2^64 - 2 wraps
HOST_OFFSETS = (0, 2 ** 32 - 3, 2 ** 64 - 2)
# device-counter entry points (an int64 tensor): 2^33 - 1 has c1 != 0 from the first counter on, so that a one-counter
# call can tell a dropped carry too
DEV_COUNTERS = (0, 2 ** 32 - 3, 2 ** 33 - 1)


# the shapes of tests/test_device_rng.py (the mutation tests of tests/test_device_rng_host.py use the smallest of each)
NORMAL_SIZES = (1, 2, 3, 4, 5, 7, 1023, 4 * 2 ** 20 + 5)      # the last: a second grid-stride round (4096 x 256 threads) and a tail
MIXMASK_SHAPES = ((1, 4), (2, 5), (64, 19), (3, 64), (5, 1))
MIXMASK_LARGE = (2 ** 19 + 3, 5)                              # 3 (2^19 + 3) > 2^20 items: a second grid-stride round
DROPOUT_SIZES = (4, 8, 1028, 4 * 1024 + 4)
DROPOUT_PS = (0.0, 0.5, 0.999)
FIELD_SIZES = (1, 3, 1023, 2 ** 20 + 3)
COWMIX_BATCHES = (1, 7, 64, 65)                               # the draw kernel's block is 64 threads
COWMIX_HW = 5                                                 # B * HW is no multiple of 4 for odd B: a tail
AFFINE_BATCHES = (1, 64, 300)                                 # the draw kernel is one block of 256 threads
AFFINE_HW = (24, 32)
AFFINE_RANGE = (15.0, 0.75, 1.25)                             # max angle (degrees), scale lo, hi
# (B, H, W), (prop_lo, prop_hi, sigma_lo, sigma_hi); the second has ragged H and W and two column blocks
END_TO_END = (((4, 128, 128), (0.3, 0.7, 4, 16)), ((3, 72, 300), (0.3, 0.7, 2, 45)), ((2, 61, 67), (0.3, 0.7, 1, 6)))


def counters(offset, n):
    """offset, offset + 1, ... (n of them) mod 2^64 as uint64"""
    return np.arange(n, dtype=np.uint64) + np.uint64(int(offset) % 2 ** 64)     # uint64 array sums wrap


def philox(ctr_u64, word2, word3, seed_u64, rounds=10, carry=True):
    """[n, 4] uint32: Philox-4x32 blocks of the counters (ctr mod 2^32, ctr >> 32, word2, word3) under the key
    (seed mod 2^32, seed >> 32).  word2 / word3: scalars or arrays of the counters' shape."""
    ctr = np.atleast_1d(np.asarray(ctr_u64, dtype=np.uint64))
    seed = int(seed_u64) % 2 ** 64
    c0, c1 = ctr & MASK32, (ctr >> np.uint64(32)) if carry else np.zeros_like(ctr)
    c2 = np.broadcast_to(np.asarray(word2, dtype=np.uint64), ctr.shape)
    c3 = np.broadcast_to(np.asarray(word3, dtype=np.uint64), ctr.shape)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2                   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u24(c):
    """float(c >> 8) * 2^-24 in fp32: exact, in [0, 1)"""
    return (c >> np.uint32(8)).astype(np.float32) * TWO_M24


def u01(c):
    """(float(c >> 8) + 1) * 2^-24 in fp32: exact, in (0, 1]"""
    return ((c >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * TWO_M24


def box_muller(words, two_pi, swap=False):
    """(z [n,4], rad [n,4]) in fp64 of the blocks `words` [n,4]: pair h = (c[2h], c[2h+1]) gives z[2h] = rad cos(ang),
    z[2h+1] = rad sin(ang) with the fp32 inputs u1 = (float(c >> 8) + 0.5f) 2^-24 and ang = two_pi * u2."""
    k1, k2 = words[:, 0::2] >> np.uint32(8), words[:, 1::2] >> np.uint32(8)
    u1 = (k1.astype(np.float32) + np.float32(0.5)) * TWO_M24
    ang = (np.float32(two_pi) * (k2.astype(np.float32) * TWO_M24)).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    co, si = (np.sin(ang), np.cos(ang)) if swap else (np.cos(ang), np.sin(ang))
    z = np.stack([rad * co, rad * si], -1).reshape(len(words), 4)
    return z, np.repeat(rad, 2, axis=1)


def normals(n, seed, offset, with_rad=False, word2=STREAM_NOISE, swap=False, **mut):
    """normal_kernel: z [n] fp64 (and the radius of each element's pair), four outputs per counter offset + q"""
    w = philox(counters(offset, (n + 3) // 4), word2, 0, seed, **mut)
    z, rad = box_muller(w, 6.283185307179586, swap)
    z, rad = z.reshape(-1)[:n], rad.reshape(-1)[:n]
    return (z, rad) if with_rad else z


def cowmix_advance(B, HW):
    return B + (B * HW + 3) // 4 + 1


def cowmix_draw(B, HW, ranges, seed, offset, word2=STREAM_PSIGMA, noise_word2=STREAM_NOISE, swap=False, **mut):
    """ssseg_cowmix_draw / ssseg_cowmix_draw_dev with ranges = (prop_lo, prop_hi, sigma_lo, sigma_hi).  A dict of
    p_unit (fp32, exact: float(c0 >> 8) 2^-24), p and sigma (fp64 values of the fp32 expressions), a (the exponent
    argument, fp64), noise and rad ([B*HW] fp64) and the advance of the counter."""
    lo, hi = np.float32(ranges[0]), np.float32(ranges[1])
    llo, lhi = np.float32(math.log(ranges[2])), np.float32(math.log(ranges[3]))
    w = philox(counters(offset, B), word2, 0, seed, **mut)
    u1, u2 = u24(w[:, 0]), u24(w[:, 1])
    p = np.float64(lo) + u1.astype(np.float64) * np.float64(hi - lo)            # hi - lo: the kernel's fp32 difference
    a = np.float64(llo) + u2.astype(np.float64) * np.float64(lhi - llo)
    z, rad = normals(B * HW, seed, int(offset) + B, True, word2=noise_word2, swap=swap, **mut)
    return dict(p_unit=u1, p=p, a=a, sigma=np.exp(a), noise=z, rad=rad, advance=cowmix_advance(B, HW))


def cowmix_reference(B, H, W, ranges, seed, offset, **mut):
    """cowmix_draw rounded to fp32 and handed to the oracle (oracle/cowmix_ref.py): adds mask, field [B,H,W], thr, std
    [B] and k_clearance, the distance of 3 max sigma to the nearest half-integer (where the window size K changes)"""
    from oracle import cowmix_ref
    d = cowmix_draw(B, H * W, ranges, seed, offset, **mut)
    sig = d['sigma'].astype(np.float32)
    mask, field, thr, _, std = cowmix_ref.cowmix_masks(d['noise'].astype(np.float32).reshape(B, H, W), sig,
                                                       d['p'].astype(np.float32))
    x = float(sig.max()) * 3.0
    return dict(d, mask=mask, field=field, thr=thr, std=std, k_clearance=abs(x - math.floor(x) - 0.5))


def affine_draw(B, H, W, max_angle, lo, hi, seed, offset, word2=STREAM_AFFINE, **mut):
    """ssseg_affine_draw_dev: (theta [B] fp32 degrees, s [B] fp32, A [B,6] fp64, A^-1 [B,6] fp64); the advance is B"""
    w = philox(counters(offset, B), word2, 0, seed, **mut)
    u1, u2 = u24(w[:, 0]), u24(w[:, 1])
    lo, hi = np.float32(lo), np.float32(hi)
    theta = np.float32(max_angle) * (np.float32(2.0) * u1 - np.float32(1.0))
    s = np.minimum(np.maximum(lo + u2 * (hi - lo), lo), hi)                     # fp32, no contraction
    assert theta.dtype == np.float32 and s.dtype == np.float32
    mats, inv = geo_ref.mats64(list(zip(theta.astype(np.float64).tolist(), s.astype(np.float64).tolist())), H, W)
    return theta, s, mats.numpy(), inv.numpy()


def mixmask_advance(B, C):
    return B * ((C + 3) // 4 + 1)


def mixmask_draw(B, C, seed, offset, word2=STREAM_KEYS, params_word2=STREAM_PARAMS, **mut):
    """ssseg_mixmask_draw_dev: (keys [B,C] int32, params [B,4] fp32, the advance of the counter)"""
    Q = (C + 3) // 4
    wk = philox(counters(offset, B * Q), word2, 0, seed, **mut)
    keys = (wk & np.uint32(0x7FFFFFFF)).astype(np.int32).reshape(B, 4 * Q)[:, :C]
    wp = philox(counters(int(offset) + B * Q, B), params_word2, 0, seed, **mut)
    return np.ascontiguousarray(keys), u24(wp), mixmask_advance(B, C)


def dropout_mask(n, p, seed, offset, word2=STREAM_DROPOUT, **mut):
    """dropout_kernel: element 4 q + e is kept where float(c[e] >> 8) 2^-24 >= p (p as fp32), counter offset + q"""
    assert n % 4 == 0
    w = philox(counters(offset, n // 4), word2, 0, seed, **mut)
    return (u24(w) >= np.float32(p)).reshape(-1)


def dropout_scale(p):
    """the fp32 quotient 1 / (1 - p) the launcher hands to the kernel"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def uniform_field(n, seed, word2=STREAM_FIELD, **mut):
    """aug_uniform_field_kernel: f[i] = 2 u01(c0) - 1 in fp32 (exact), counter i"""
    w = philox(counters(0, n), word2, 0, seed, **mut)
    return u01(w[:, 0]) * np.float32(2.0) - np.float32(1.0)


def iso_uniforms(n_img, HW, seed, word3=WORD3_ISO, **mut):
    """aug_iso_finish_kernel: [n_img, HW, 3] fp32, u01 of (c0, c1, c2) of pixel i of image n: counter i, c2 = n"""
    ctr = np.tile(counters(0, HW), n_img)
    img = np.repeat(np.arange(n_img, dtype=np.uint64), HW)
    w = philox(ctr, img, word3, seed, **mut)
    return u01(w[:, :3]).reshape(n_img, HW, 3)


def iso_normal(u, swap=False):
    """the kernel's sqrtf(-2 logf(u1)) cosf(6.2831853f * u2) in fp64 from the fp32 inputs u[..., 0], u[..., 1]"""
    ang = (np.float32(6.2831853) * u[..., 1]).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u[..., 0].astype(np.float64))) * (np.sin(ang) if swap else np.cos(ang))


def iso_reference(img, color_std, seed, swap=False, **mut):
    """[n,3,H,W] fp64: oracle/augment_ref.iso_finish of the images [n,H,W,3] under hue noise color_std[n] times the
    host-predicted normal of each pixel (intensity 0: no luminance noise); color_std[n] None: ISO off (ToFloat alone)"""
    from oracle import augment_ref
    n, H, W, _ = img.shape
    nrm = iso_normal(iso_uniforms(n, H * W, seed, **mut), swap).reshape(n, H, W)
    return np.stack([augment_ref.iso_finish(img[i], dict(iso=0)) if s is None else
                     augment_ref.iso_finish(img[i], dict(iso=1), hue_noise=nrm[i] * s) for i, s in enumerate(color_std)])


# ---- comparators: each returns the largest error / bound ratio (<= 1 passes) and asserts it -------------------------
def _ratio(err, bound):
    """max err / bound; where the bound is 0 the values must be equal"""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(err), r, np.inf)                                   # NaN or inf from the device fails
    return float(r.max())


def _worst(what, err, bound, ratio):
    i = int(np.argmax(np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf)))
    return f'{what}: error / bound = {ratio:.3f} at element {i} (error {err.reshape(-1)[i]:.3e}, bound {bound.reshape(-1)[i]:.3e})'


def check_exact(got, ref, what=''):
    """bit-for-bit equality of two integer, bool or float arrays (floats by value and dtype)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, (f'{what}: {bad.size} of {got.size} differ, first at {int(bad[0])}: '
                           f'{got.reshape(-1)[bad[0]]!r} != {ref.reshape(-1)[bad[0]]!r}')
    return 0.0


def check_normals(got, z_ref, rad_ref, what=''):
    """|z_dev - z_ref| <= 2^-21 (|z_ref| + rad_ref), and |z| <= 5.89"""
    got = np.asarray(got, np.float64)
    assert got.shape == z_ref.shape, (what, got.shape, z_ref.shape)
    err = np.abs(got - z_ref)
    bound = 2.0 ** -21 * (np.abs(z_ref) + rad_ref)
    r = _ratio(err, bound)
    assert r <= 1.0, _worst(what, err, bound, r)
    assert got.size == 0 or float(np.abs(got).max()) <= 5.89, (what, float(np.abs(got).max()))
    return r


def ulp32(x):
    """the spacing of fp32 at |x| (of the fp32 nearest to x)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_ulp(got, ref64, what='', ulps=1.0):
    """fp32 `got` within `ulps` fp32 ulps of the fp64 reference"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(ref64), (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - ref64)
    bound = ulps * ulp32(ref64)
    r = _ratio(err, bound)
    assert r <= 1.0, _worst(what, err, bound, r)
    return r


def check_sigma(got, sigma_ref, a_ref, sigma_lo, sigma_hi, what=''):
    """relative error <= 2^-23 (4 + 2 |a|), and sigma_lo (1 - 2^-20) <= sigma <= sigma_hi (1 + 2^-20)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == sigma_ref.shape, (what, got.dtype, got.shape)
    g = got.astype(np.float64)
    err = np.abs(g - sigma_ref)
    bound = 2.0 ** -23 * (4.0 + 2.0 * np.abs(a_ref)) * sigma_ref
    r = _ratio(err, bound)
    assert r <= 1.0, _worst(what, err, bound, r)
    assert (g >= sigma_lo * (1 - 2.0 ** -20)).all() and (g <= sigma_hi * (1 + 2.0 ** -20)).all(), (what, g.min(), g.max())
    return r


def check_affine(got, ref64, H, W, what=''):
    """[B,6] fp32 matrix against geo_ref.mats64: entries 0, 1, 3, 4 within 1 fp32 ulp, the translations 2 and 5 within
    2^-23 max(1, cx, cy)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref64.shape, (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - ref64)
    bound = ulp32(ref64)
    bound[:, [2, 5]] = 2.0 ** -23 * max(1.0, (W - 1) / 2.0, (H - 1) / 2.0)
    r = _ratio(err, bound)
    assert r <= 1.0, _worst(what, err, bound, r)
    return r


def check_masks(mask, thr, ref, what=''):
    """device mask [B,H,W] and thr [B] against cowmix_reference: equal masks outside the band
    |field_ref - thr_ref| < 4E + 1e-5 std, at most 0.2 % of the pixels inside it, thr within 1e-5 |thr| + 2E.
    Returns (fraction of the pixels in the band, differing pixels inside it, thr error / bound)."""
    mask, thr = np.asarray(mask, np.float32), np.asarray(thr, np.float64)
    assert mask.shape == ref['mask'].shape and thr.shape == ref['thr'].shape, (what, mask.shape, thr.shape)
    assert set(np.unique(mask).tolist()) <= {0.0, 1.0}, what
    tref, std = ref['thr'].astype(np.float64), ref['std'].astype(np.float64)
    band = np.abs(ref['field'].astype(np.float64) - tref[:, None, None]) < (4 * E_NORMAL + 1e-5 * std)[:, None, None]
    diff = mask != ref['mask']
    frac = float(band.mean())
    assert frac <= 0.002, f'{what}: {frac:.5f} of the pixels lie in the band'
    outside = int((diff & ~band).sum())
    assert outside == 0, f'{what}: {outside} pixels outside the band differ ({int(diff.sum())} in all)'
    err, bound = np.abs(thr - tref), 1e-5 * np.abs(tref) + 2 * E_NORMAL
    r = _ratio(err, bound)
    assert r <= 1.0, _worst(what + ' thr', err, bound, r)
    return frac, int((diff & band).sum()), r


def check_levels(got, ref, what=''):
    """test_iso_finish's tolerance: every value within one 8-bit level, more than half of them equal"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert d.shape == np.shape(ref) and d.max() <= 1.0 / 255 + 1e-6 and (d < 1e-6).mean() > 0.5, \
        f'{what}: largest difference {d.max() * 255:.3f} levels, {float((d < 1e-6).mean()):.4f} equal'
    return float(d.max() * 255), float((d < 1e-6).mean())
