"""TEST INFRASTRUCTURE ONLY (tests/ may import this; the product path never does).

NumPy restatement of the device augmentation kernels (csrc/augment.hip, data/device_augment.py), which restate the
reference config's albumentations pipelines (configs/default_config.py:179-212).  albumentations and cv2 are absent
from this image, so parity with the reference pipeline itself is UNPINNED: this oracle pins the kernels' own
arithmetic (OpenCV pixel-centre bilinear / nearest sampling, reflect-101 borders, the uint8-grid colour ops, cv2 /
scipy Gaussian taps, RGB <-> HLS / 8-bit HSV conversions), not albumentations' outputs.

Keywords for the per-pixel tests (tests/augment_cases.py); the defaults give the results this file always gave:
  * dtype: np.float64 (the expected value) or np.float32 -- the same restatement with every operation rounded to fp32,
    unfused.  fp32 results only measure the restatement's own fp32-vs-fp64 deviation; they are never expected values.
  * details: also return a dict with the value before every rounding step (the argument of each rint / floor), the
    sampling coordinates, and for `poisson` the CDF steps.  Rounding records are tuples (name, value, kind, rounded,
    clipped): kind 'rint' / 'floor', or 'cont' where the floor only selects a branch of a continuous function;
    clipped says the value goes through clip(., 0, 255) before the rounding.
  * mut: names of deliberate mistakes, for the mutation tests alone (tests/test_augment_exact_host.py): the comparators
    must reject a reference built with them.
"""
import numpy as np


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def reflect_sym(i, n):
    i = np.asarray(i)
    period = 2 * n
    i = np.where(i < 0, -i - 1, i) % period
    return np.where(i >= n, period - 1 - i, i)


def _round(v, kind, mut=()):
    if 'trunc' in mut:
        return np.floor(v)
    if 'half_up' in mut and kind == 'rint':
        return np.floor(v + 0.5)
    return np.rint(v) if kind == 'rint' else np.floor(v)


def distort(p, S, gmap, field, dtype=np.float64, out_hw=None):
    """Crop-grid pixel coordinates after the sample's distortion (ssseg_aug_warp_params.distort)."""
    f = np.dtype(dtype).type
    Ho, Wo = out_hw or (S, S)
    y, x = np.mgrid[0:Ho, 0:Wo].astype(dtype)
    if p['distort'] == 1:   # ElasticTransform: Minv (x + dx, y + dy)
        field = np.asarray(field, dtype)
        ex, ey = x + field[..., 0], y + field[..., 1]
        m = [f(v) for v in p['m']]
        return m[0] * ex + m[1] * ey + m[2], m[3] * ex + m[4] * ey + m[5]
    if p['distort'] == 2:   # GridDistortion: separable axis maps
        gmap = np.asarray(gmap, dtype)
        return np.broadcast_to(gmap[:Wo][None, :], (Ho, Wo)), np.broadcast_to(gmap[Wo:Wo + Ho][:, None], (Ho, Wo))
    if p['distort'] == 3:   # OpticalDistortion (cv2.initUndistortRectifyMap, k1 = k2 = k)
        cx, cy, fx, fy, k = f(p['cx']), f(p['cy']), f(p['fx']), f(p['fy']), f(p['k'])
        u, v = (x - cx) / fx, (y - cy) / fy
        r2 = u * u + v * v
        kr = 1 + k * r2 + k * r2 * r2
        return fx * u * kr + cx, fy * v * kr + cy
    return x, y


def mask_at(mask, mx, my, border, clamp=False):
    """Nearest-sampled mask CxHoxWo in [0, 255] at the integer source pixels (mx, my) under the border rule."""
    H, W = mask.shape[:2]
    if border == 1:
        return mask[reflect101(my, H), reflect101(mx, W)].astype(np.float64).transpose(2, 0, 1)
    ok = (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
    v = mask[np.clip(my, 0, H - 1), np.clip(mx, 0, W - 1)]
    return (v if clamp else np.where(ok[..., None], v, 0)).astype(np.float64).transpose(2, 0, 1)


def warp(img, mask, p, S, gmap=None, field=None, dtype=np.float64, details=False, out_hw=None, mut=()):
    """One sample: image HxWx3 uint8 -> SxSx3 float on the uint8 grid (bilinear), mask HxWxC uint8 -> CxSxS [0, 1].
    out_hw = (Ho, Wo): a non-square output (gmap then holds Wo x-entries followed by Ho y-entries)."""
    f = np.dtype(dtype).type
    H, W = img.shape[:2]
    Ho, Wo = out_hw or (S, S)
    qx, qy = distort(p, S, gmap, field, dtype, out_hw)
    a = [f(v) for v in p['a']]
    sx, sy = a[0] * qx + a[1] * qy + a[2], a[3] * qx + a[4] * qy + a[5]
    x0, y0 = np.floor(sx), np.floor(sy)
    lx, ly = sx - x0, sy - y0
    if 'swap_lxly' in mut:
        lx, ly = ly, lx
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    if 'tap_shift' in mut:
        x0 = x0 + 1
    refl = reflect_sym if 'reflect_edge' in mut else reflect101
    out = np.zeros((Ho, Wo, 3), dtype)
    for t in range(4):
        xx, yy = x0 + (t & 1), y0 + (t >> 1)
        wgt = (lx if t & 1 else 1 - lx) * (ly if t >> 1 else 1 - ly)
        if p['border'] == 1:
            xx, yy = refl(xx, W), refl(yy, H)
            ok = np.ones_like(wgt, bool)
        else:
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            if 'border_clamp' in mut:
                ok = np.ones_like(wgt, bool)
            xx, yy = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
        out += np.where(ok, wgt, f(0))[..., None] * img[yy, xx].astype(dtype)
    pre = out
    out = _round(np.clip(pre, 0, 255), 'rint', mut)
    if 'channels' in mut:
        out = out[..., ::-1]
    m = None
    if mask is not None:
        rnd = (lambda v: np.floor(v + f(0.5))) if 'nearest_half_up' in mut else np.rint
        mx, my = rnd(sx).astype(np.int64), rnd(sy).astype(np.int64)
        if p['border'] == 1:
            mx, my = refl(mx, W), refl(my, H)
            m = mask[my, mx].astype(np.float64) / 255.0
        else:
            ok = (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
            if 'border_clamp' in mut:
                ok = np.ones_like(ok)
            m = np.where(ok[..., None], mask[np.clip(my, 0, H - 1), np.clip(mx, 0, W - 1)], 0) / 255.0
        m = m.transpose(2, 0, 1)
        if 'channels' in mut:
            m = m[::-1]
    if details:
        return out, m, dict(sx=sx, sy=sy, rounds=[('bilinear', pre, 'rint', out, True)])
    return out, m


def rgb2hsv8(r, g, b, rec=None, mut=()):
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    v = mx
    s = np.where(mx > 0, 255 * d / np.where(mx > 0, mx, 1), 0)
    dd = np.where(d > 0, d, 1)
    hd = np.where(mx == r, 60 * (g - b) / dd, np.where(mx == g, 120 + 60 * (b - r) / dd, 240 + 60 * (r - g) / dd))
    hd = np.where(d > 0, np.where(hd < 0, hd + 360, hd), 0)
    h = _round(hd if 'hue360' in mut else hd * 0.5, 'rint', mut)      # hue360: the hue kept in degrees, wrapped at 360
    if rec is not None:
        rec += [('hsv.h', hd * 0.5, 'rint', h, False), ('hsv.s', s, 'rint', _round(s, 'rint', mut), False),
                ('hsv.v', v, 'rint', _round(v, 'rint', mut), False)]
    h = np.where(h >= 360, h - 360, h) if 'hue360' in mut else np.where(h >= 180, h - 180, h)
    return h, _round(s, 'rint', mut), _round(v, 'rint', mut)


def hsv82rgb(h, s, v, rec=None, mut=()):
    hd, sf = h if 'hue360' in mut else h * 2, s / 255
    c = v * sf
    hp = hd / 60
    x = c * (1 - np.abs(np.fmod(hp, 2) - 1))
    m = v - c
    sec = np.floor(hp).astype(np.int64) % 6
    z = np.zeros_like(c)
    r1 = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [c, x, z, z, x], c)
    g1 = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [x, c, c, x, z], z)
    b1 = np.select([sec == 0, sec == 1, sec == 2, sec == 3, sec == 4], [z, z, x, c, c], x)
    pre = np.stack([r1 + m, g1 + m, b1 + m], -1)
    out = _round(np.clip(pre, 0, 255), 'rint', mut)
    if rec is not None:
        rec += [('rgb.sector', hp, 'cont', np.floor(hp), False), ('rgb.out', pre, 'rint', out, True)]
    return out[..., 0], out[..., 1], out[..., 2]


def color(img, p, dtype=np.float64, details=False, mut=()):
    """ssseg_aug_color on one HxWx3 [0, 255] image (float64)."""
    f = np.dtype(dtype).type
    rec = []

    def stage(name, pre, kind='floor'):
        pre = np.stack(pre, -1)
        out = _round(np.clip(pre, 0, 255), kind, mut)
        rec.append((name, pre, kind, out, True))
        return out[..., 0], out[..., 1], out[..., 2]

    r, g, b = (img[..., i].astype(dtype) for i in range(3))
    if p.get('bc'):
        al, be = f(p['alpha']), f(p['beta'])
        r, g, b = stage('bc', [t * al + be * 255 for t in (r, g, b)])
    if p.get('gray'):   # albumentations to_gray = cv2 RGB2GRAY -> GRAY2RGB; OpenCV's 8-bit RGB2GRAY is the Q14 fixed
        # point CV_DESCALE(R*4899 + G*9617 + B*1868, 14) (coefficients 0.299 / 0.587 / 0.114 scaled by 2^14)
        rec.append(('gray', None, 'mix', None, False))
        ri, gi, bi = (t.astype(np.int64) for t in (r, g, b))
        y = ((ri * 4899 + gi * 9617 + bi * 1868 + 8192) >> 14).astype(dtype)
        r = g = b = y
    if p.get('rgb'):
        r, g, b = stage('rgb', [t + f(s) for t, s in zip((r, g, b), p['shift'])])
    if p.get('hsv'):
        sh = [f(v) for v in p['hsv_shift']]
        rec.append(('hsv', None, 'mix', None, False))
        h, s, v = rgb2hsv8(r, g, b, rec, mut)
        h = np.fmod(h + sh[0], 360 if 'hue360' in mut else 180)
        hw = np.where(h < 0, h + (360 if 'hue360' in mut else 180), h)
        h = np.floor(hw)
        rec.append(('hsv.shift_h', hw, 'floor', h, False))
        sv = _round(np.clip(np.stack([s + sh[1], v + sh[2]], -1), 0, 255), 'floor', mut)
        rec.append(('hsv.shift_sv', np.stack([s + sh[1], v + sh[2]], -1), 'floor', sv, True))
        r, g, b = hsv82rgb(h, sv[..., 0], sv[..., 1], rec, mut)
    out = np.stack([r, g, b], -1)
    if 'channels' in mut:
        out = out[..., ::-1]
    return (out, dict(rounds=rec)) if details else out


def blur(x, radius, weights, sym=False, round8=False, dtype=np.float64, details=False, mut=()):
    """Separable Gaussian of one HxWxC plane set (horizontal, then vertical)."""
    x = np.asarray(x, dtype)
    if radius == 0:
        return (x.copy(), dict(rounds=[])) if details else x.copy()
    H, W = x.shape[:2]
    refl = reflect_sym if bool(sym) != ('reflect_swap' in mut) else reflect101
    w = np.asarray(weights[:2 * radius + 1], dtype)
    if 'taps_reversed' in mut:
        w = w[::-1]
    sh = 1 if 'tap_shift' in mut else 0
    tmp = np.zeros_like(x, dtype=dtype)
    for k in range(-radius, radius + 1):
        tmp += w[k + radius] * x[:, refl(np.arange(W) + k + sh, W)]
    out = np.zeros_like(tmp)
    if 'skip_vert_h1' in mut and H == 1:
        out = tmp
    else:
        for k in range(-radius, radius + 1):
            out += w[k + radius] * tmp[refl(np.arange(H) + k + sh, H)]
    res = _round(np.clip(out, 0, 255), 'rint', mut) if round8 else out
    if details:
        return res, dict(rounds=[('blur', out, 'rint', res, True)] if round8 else [], pre=out)
    return res


def rgb2hls(r, g, b):
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    l = 0.5 * (mx + mn)
    dd = np.where(d > 1e-12, d, 1)
    s = np.where(d > 1e-12, np.where(l < 0.5, d / np.where(mx + mn > 0, mx + mn, 1), d / np.where(2 - mx - mn > 0,
                                                                                               2 - mx - mn, 1)), 0)
    h = np.where(mx == r, 60 * (g - b) / dd, np.where(mx == g, 120 + 60 * (b - r) / dd, 240 + 60 * (r - g) / dd))
    h = np.where(d > 1e-12, np.where(h < 0, h + 360, h), 0)
    return h, l, s


def _hls_c(p, q, t):
    t = np.where(t < 0, t + 360, t)
    t = np.where(t >= 360, t - 360, t)
    return np.select([t < 60, t < 180, t < 240], [p + (q - p) * t / 60, q, p + (q - p) * (240 - t) / 60], p)


def hls2rgb(h, l, s):
    q = np.where(l < 0.5, l * (1 + s), l + s - l * s)
    p = 2 * l - q
    r, g, b = _hls_c(p, q, h + 120), _hls_c(p, q, h), _hls_c(p, q, h - 120)
    gray = s <= 0
    return np.where(gray, l, r), np.where(gray, l, g), np.where(gray, l, b)


def iso_finish(img, p, hue_noise=None, lum_noise=None, dtype=np.float64, details=False):
    """ISONoise with the given per-pixel hue noise (already scaled) and Poisson luminance counts, then ToFloat
    (NCHW [0, 1]).  hue_noise / lum_noise None: no noise (the conversion chain alone).  details: also the uint8-grid
    levels HxWx3 (the kernel's ToFloat is float(level) * (1.f / 255.f)) and the floor's arguments."""
    x = img.astype(dtype)
    rec = []
    if p.get('iso'):
        h, l, s = rgb2hls(x[..., 0] / 255, x[..., 1] / 255, x[..., 2] / 255)
        if hue_noise is not None:
            h = h + np.asarray(hue_noise, dtype)
            h = np.where(h < 0, h + 360, h)
            h = np.where(h > 360, h - 360, h)
        if lum_noise is not None:
            l = l + np.asarray(lum_noise, dtype) / 255 * (1 - l)
        r, g, b = hls2rgb(h, l, s)
        pre = np.stack([t * 255 for t in (r, g, b)], -1)
        x = np.floor(np.clip(pre, 0, 255))
        rec.append(('iso.out', pre, 'floor', x, True))
    out = (x / 255).transpose(2, 0, 1)
    return (out, dict(levels=x, rounds=rec)) if details else out


def lum_stats(img):
    """aug_lum_stats_kernel of one HxWx3 [0, 255] image: (sum L, sum L^2) in fp64 of L = (max + min) / 2, where the
    division by 255 and the max / min are fp32 and the widening comes after them."""
    x = np.asarray(img, np.float32) / np.float32(255)
    l = 0.5 * (x.max(-1).astype(np.float64) + x.min(-1).astype(np.float64))
    return float(l.sum()), float((l * l).sum())


def iso_lambda(s1, s2, HW, intensity, dtype=np.float64):
    """aug_iso_finish_kernel's Poisson mean from the fp64 sums: min(sqrt(var) intensity 255, 80); with np.float32 the
    square root is rounded to fp32 first and the products are fp32, as the kernel writes them."""
    f = np.dtype(dtype).type
    m = s1 / HW
    var = max(s2 / HW - m * m, 0.0)
    return min(f(np.sqrt(var)) * f(intensity) * f(255), f(80))


def poisson(lam, u, dtype=np.float64, details=False):
    """The kernel's Poisson(lam) by inversion for the uniforms u: p_0 = F_0 = exp(-lam); while u > F_k and k < 1024:
    k += 1, p_k = p_{k-1} lam / k, F_k = F_{k-1} + p_k, leaving where p_k < 1e-30 and k > lam.  Returns the counts
    (and with details the CDF steps F_0 .. F_K, K, and which pixels left through the exit, u > F_K)."""
    f = np.dtype(dtype).type
    lam = f(lam)
    u = np.asarray(u, dtype)
    p = np.exp(-lam)
    F = [p]
    k = 0
    while k < 1024:
        k += 1
        p = p * (lam / f(k))
        F.append(F[-1] + p)
        if p < f(1e-30) and f(k) > lam:
            break
    F = np.array(F, dtype)
    count = np.minimum(np.searchsorted(F, u, side='left'), k).astype(dtype)
    return (count, dict(F=F, K=k, exited=u > F[k])) if details else count
