"""Case tables, expected values and comparators of the per-pixel augmentation tests (tests/test_augment_exact.py on the
device, tests/test_augment_exact_host.py on the oracle alone).

The rule, wherever the inputs are not exact by construction.  Every rounding step of a kernel (rint, floor, the nearest
pixel of the mask, the step of the Poisson CDF) has a decision value: the number that is rounded.  The restatement of
oracle/augment_ref.py evaluates it in fp64 (the expected value) and again with every operation rounded to fp32,
unfused; eps of a decision value is 4 x the largest |fp32 - fp64| of that value over the sample (taken where the two
runs still agree on every earlier rounding of the chain, so that a flipped earlier step does not count as deviation of
a later one).  The 4 is the margin the sliding-window tests give the restatement's own deviation; augment.hip is built
with contraction on, and a fused multiply-add rounds once where the unfused restatement rounds twice, so the device
stays within what the deviation measures.  An element is undecided if a decision value feeding it lies within eps
(strictly: eps = 0, exact arithmetic, leaves nothing undecided) of a boundary of its rounding: k + 0.5 for rint, an
integer for floor, a CDF step for the Poisson count, a half-integer coordinate for the mask.  Decided elements must
equal the fp64 oracle bit for bit.  Undecided ones must be one of the two neighbouring outcomes: the two sides of the
boundary where the last rounding is the only close one, within one level otherwise; for the mask the value at one of
the candidate source pixels; for the Poisson count +-1.  The undecided share per sample is capped (CAP_*): the cap is
asserted on the oracle alone (`*_expected`), so a case that exceeds it fails on the host before any device run.

One refinement, for the 8-bit HSV conversion alone (EXACT_TIES): its hue and saturation are rint(integer * integer /
integer) -- exact integers, one correctly rounded division, then exact additions and a halving -- so a value that both
restatements put exactly on k + 0.5 is a tie of the real quotient, which every correctly rounded division returns:
it is decided (round-half-even), not undecided.  On the colour lattice 5-6 % of the pixels are such ties (channel
values that are multiples of 5); they are where round-half-even is pinned, and counting them as undecided would let
round-half-up pass.
"""
import numpy as np

from oracle import augment_ref as R

CAP_IMAGE, CAP_MASK, CAP_POISSON = 0.02, 0.005, 0.001
EXACT_TIES = ('hsv.h', 'hsv.s')
MARGIN = 4.0
INV255 = np.float32(1.0 / 255.0)


def to_float(levels):
    """the kernels' ToFloat: float(level) * (1.f / 255.f), bit for bit"""
    return np.asarray(levels, np.float32) * INV255


# ---- the rule --------------------------------------------------------------------------------------------------------
def boundary(v, kind, clipped):
    """(distance of v to the nearest boundary of its rounding, the outcome below it, the outcome above it); with
    clip(., 0, 255) before the rounding only the boundaries inside the clip range are boundaries"""
    v = np.asarray(v, np.float64)
    if kind == 'floor':
        b = np.rint(v)
        lo, hi, valid = b - 1, b, (b >= 1) & (b <= 255) if clipped else np.ones(v.shape, bool)
    else:
        b = np.floor(v) + 0.5
        lo, hi, valid = b - 0.5, b + 0.5, (b >= 0.5) & (b <= 254.5) if clipped else np.ones(v.shape, bool)
    return np.where(valid, np.abs(v - b), np.inf), lo, hi


def _pix(a):
    """per-pixel view of a per-element flag: any over the channels, kept as a last axis of 1"""
    return a.any(-1, keepdims=True) if a.ndim == 3 else a[..., None]


def decide(r64, r32, shape, strict=True):
    """The rule on the rounding records of one sample (fp64 and fp32 runs of the same chain) for an output of `shape`
    HxWxC.  Returns dict(und, lo, hi, eps, dist): und the undecided elements, lo / hi the two admissible outcomes where
    only the last rounding is close (NaN elsewhere), eps per record name, dist the last record's boundary distance."""
    und, same = np.zeros(shape, bool), np.ones(shape, bool)
    lo = hi = np.full(shape, np.nan)
    dist = np.full(shape, np.inf)
    eps = {}
    live = [(a, b) for a, b in zip(r64, r32) if a[2] != 'cont']
    for idx, ((name, v64, kind, p64, clipped), (_, v32, _, p32, _)) in enumerate(live):
        if kind == 'mix':      # the channels mix from here on (gray, HSV): flags become per pixel
            und, same = np.broadcast_to(_pix(und), shape).copy(), np.broadcast_to(~_pix(~same), shape).copy()
            continue
        chan = v64.shape == tuple(shape)
        s = same if chan else same.all(-1) if v64.ndim == 2 else np.broadcast_to(~_pix(~same), v64.shape)
        dev = float(np.abs(v32.astype(np.float64) - v64)[s].max()) if s.any() else 0.0
        e = eps[name] = max(eps.get(name, 0.0), MARGIN * dev)
        d, l, h = boundary(v64, kind, clipped)
        near, differ = d < e, p32.astype(np.float64) != p64
        if name in EXACT_TIES:
            near &= ~((d == 0) & (v32.astype(np.float64) == v64))
        assert not (strict and (differ & s & ~near).any()), f'{name}: fp32 and fp64 round apart outside eps'
        if chan:
            if idx == len(live) - 1:
                first = near & ~und
                lo, hi, dist = np.where(first, l, np.nan), np.where(first, h, np.nan), d
            und, same = und | near, same & ~differ
        else:
            und, same = und | _pix(near), same & ~_pix(differ)
    return dict(und=und, lo=lo, hi=hi, eps=eps, dist=dist)


def check_levels(got, ref, dec, cap, what):
    """`got` against the fp64 levels `ref` under the rule (dec = decide(...)).  Returns (largest boundary distance of a
    differing element / eps of the last rounding, undecided share)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    und = dec['und']
    share = float(und.mean())
    assert share <= cap, f'{what}: {share:.5f} of the values undecided (cap {cap})'
    bad = np.flatnonzero((got != ref).reshape(-1) & ~und.reshape(-1))
    assert bad.size == 0 and np.array_equal(got[~und], ref[~und]), (
        f'{what}: {bad.size} decided values differ, first at {int(bad[0])}: {got.reshape(-1)[bad[0]]} != '
        f'{ref.reshape(-1)[bad[0]]}')
    two = ~np.isnan(dec['lo'])
    ok = np.where(two, (got == dec['lo']) | (got == dec['hi']), np.abs(got - ref) <= 1.0)
    assert ok[und].all(), f'{what}: {int((~ok & und).sum())} undecided values are not a neighbouring outcome'
    diff = (got != ref) & two
    e = max(dec['eps'].values()) if dec['eps'] else 0.0
    return (float(dec['dist'][diff].max()) / e if diff.any() else 0.0), share


def check_close(got, ref64, ref32, what):
    """an unrounded output: |got - ref64| <= 4 max |ref32 - ref64|; returns the ratio (0 where both are exact)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    e = MARGIN * float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    err = float(np.abs(got - ref64).max())
    assert err <= e, f'{what}: error {err:.3e} beyond eps {e:.3e}'
    return err / e if e > 0 else 0.0


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---- warp ------------------------------------------------------------------------------------------------------------
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def wp(a, border=1, distort=0, field=0, m=IDENT, k=0.0, cx=0.0, cy=0.0, fx=1.0, fy=1.0):
    f32 = lambda v: [float(np.float32(t)) for t in v]      # noqa: E731  (what the fp32 record holds)
    return dict(a=f32(a), border=border, distort=distort, field=field, m=f32(m), k=float(np.float32(k)), cx=float(cx),
                cy=float(cy), fx=float(fx), fy=float(fy))


def _image(rng, n, H, W, C=3):
    return rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)


def _mask(n, H, W, Cm):
    """per-channel distinct values: channel c of pixel (n, y, x) identifies all four"""
    i = np.arange(n * H * W, dtype=np.int64).reshape(n, H, W, 1)
    return ((i * 7 + np.arange(Cm) * 37 + 1) % 251 + np.arange(Cm)).astype(np.uint8)


def _case(name, img, params, Ho, Wo, Cm=2, gmaps=None, fields=None, exact=True, exact_image=None):
    n, H, W, _ = img.shape
    return dict(name=name, img=img, mask=_mask(n, H, W, Cm) if Cm else None, params=params, Ho=Ho, Wo=Wo,
                gmaps=np.zeros((n, Wo + Ho), np.float32) if gmaps is None else gmaps,
                fields=np.zeros((1, Ho, Wo, 2), np.float32) if fields is None else fields, exact=exact,
                exact_image=exact if exact_image is None else exact_image)


def _dyadic(rng, shape, lo, hi, step=0.125):
    return (rng.integers(int(lo / step), int(hi / step) + 1, size=shape) * step).astype(np.float32)


def warp_exact_cases():
    """every fp32 operation is exact: dyadic matrices, maps and fields, weights multiples of 1/8, uint8 images"""
    rng = np.random.default_rng(101)
    H, W = 6, 8
    img = _image(rng, 2, H, W)
    cases = [
        _case('identity', img, [wp(IDENT, 1), wp(IDENT, 0)], H, W, Cm=1),
        _case('hflip', img, [wp([-1, 0, W - 1, 0, 1, 0], 1), wp([-1, 0, W - 1, 0, 1, 0], 0)], H, W, Cm=2),
        # 2x decimation, translation 0.5: four-pixel means (ties of the image), half-integer mask coordinates
        _case('decimate', img, [wp([2, 0, 0.5, 0, 2, 0.5], 1), wp([2, 0, 0.5, 0, 2, 0.5], 0)], H // 2 + 1, W // 2 + 1, Cm=3),
        _case('magnify', img, [wp([0.5, 0, -0.25, 0, 0.5, -0.25], 1), wp([0.5, 0, -0.25, 0, 0.5, -0.25], 0)], 2 * H, 2 * W,
              Cm=5),
        _case('rot90', img, [wp([0, 1, 0, -1, 0, H - 1], 1), wp([0, 1, -0.5, -1, 0, H - 0.5], 0)], W, H, Cm=2),
        _case('shear', img, [wp([1, 0.25, 0, 0, 1, 0], 1), wp([1, 0.25, -1, 0.125, 1, 0], 0)], H, W, Cm=2),
    ]
    # the whole window 0.5, 1.5 and 3.5 image periods outside, on either side of both axes, both borders
    px, py = 2 * W - 2, 2 * H - 2
    ps = [wp([1, 0, sgn * k * px + 0.25, 0, 1, -sgn * k * py + 0.375], border)
          for border in (1, 0) for k in (0.5, 1.5, 3.5) for sgn in (1, -1)]
    cases.append(_case('periods', _image(rng, len(ps), H, W), ps, H, W, Cm=2))
    # H = 1 and W = 1 sources: the n == 1 branch of reflect-101
    ps = [wp([0.5, 0, -3.25, 0, 0.25, -1.5], 1), wp([0.5, 0, -1.25, 0, 0.5, -0.75], 0), wp([1, 0, 20, 0, 1, -30], 1)]
    cases.append(_case('H=1', _image(rng, 3, 1, 5), ps, 4, 9, Cm=2))
    cases.append(_case('W=1', _image(rng, 3, 5, 1), ps, 9, 4, Cm=3))
    # output widths around the 128-wide block, one and three rows
    for Wo in (1, 127, 128, 129, 257):
        for Ho in (1, 3):
            ps = [wp([0.5, 0, -3.25, 0.125, 0.5, -1.25], 1), wp([0.125, 0, -1.5, 0, 1, -0.5], 0)]
            cases.append(_case(f'Wo={Wo} Ho={Ho}', _image(rng, 2, 7, 9), ps, Ho, Wo, Cm=2))
    # batches of three that differ in kind, border and matrix; elastic field indices a non-identity permutation of the
    # sample index into a buffer with more fields than elastic samples
    Ho, Wo = 5, 12
    fields = _dyadic(rng, (4, Ho, Wo, 2), -3, 3)
    gm = np.zeros((3, Wo + Ho), np.float32)
    for i in range(3):
        gm[i, :Wo] = np.cumsum(_dyadic(rng, Wo, 0.5, 1.5)) - 1 - i
        gm[i, Wo:] = np.cumsum(_dyadic(rng, Ho, 0.5, 1.5)) - 2 + i
    m1, m2 = [1, 0.25, 0.5, 0, 1, -0.5], [1, 0, -1, -0.5, 1, 2]
    cases.append(_case('batch elastic/grid/elastic', _image(rng, 3, 7, 9),
                       [wp([1, 0, -1, 0, 1, 0.5], 1, 1, 2, m1), wp([0.5, 0, 0.25, 0, 1, 0], 0, 2),
                        wp([1, 0.5, 0, 0, 1, -2], 0, 1, 0, m2)], Ho, Wo, Cm=5, gmaps=gm, fields=fields))
    cases.append(_case('batch grid/none/elastic', _image(rng, 3, 7, 9),
                       [wp([1, 0, 0, 0.25, 1, 0], 1, 2), wp([-1, 0, 9.5, 0, 0.5, 0.25], 0),
                        wp([1, 0, 0.5, 0, 1, 0], 1, 1, 1, m2)], Ho, Wo, Cm=3, gmaps=gm[::-1].copy(), fields=fields))
    # optical at S = 16, fx = fy = 16, integer centres: the coordinates are exact in fp32 (every intermediate fits in
    # 24 bits), hence the mask; the bilinear weights are multiples of 2^-17, not of 1/8, so their products are not
    # exact and the image of this case goes by the rule
    ps = [wp(IDENT, 1, 3, k=0.5, cx=8, cy=7, fx=16, fy=16), wp([1, 0, -2, 0, 1, 1], 0, 3, k=-0.25, cx=6, cy=9, fx=16, fy=16),
          wp([-1, 0, 15, 0, 1, 0], 1)]
    cases.append(_case('batch optical/optical/none', _image(rng, 3, 16, 16), ps, 16, 16, Cm=1, exact_image=False))
    return cases


def _host_affine(rng, S_w, S_h, H, W, grow):
    """rotation o crop o flip as the host composes them, with a crop window `grow` times the image (so that the
    sampling point leaves the image for a large share of the pixels)"""
    from data import device_augment as DA
    Rm = DA.rotation_matrix(rng.uniform(-15, 15), W / 2 - 0.5, H / 2 - 0.5)
    w, h = grow * W * rng.uniform(0.8, 1.0), grow * H * rng.uniform(0.8, 1.0)
    x0, y0 = (W - w) / 2 + rng.uniform(-4, 4), (H - h) / 2 + rng.uniform(-4, 4)
    C = [w / S_w, 0.0, 0.5 * w / S_w - 0.5 + x0, 0.0, h / S_h, 0.5 * h / S_h - 0.5 + y0]
    F = [-1.0, 0.0, S_w - 1.0, 0.0, 1.0, 0.0] if rng.random() < 0.5 else IDENT
    return DA._compose(DA._affine_inv(Rm), DA._compose(C, F))


def warp_general_cases():
    """all four kinds with random parameters in the host's ranges, both borders, the sampling point outside the image
    for at least 20 % of the pixels of every sample, |coordinate| <= 8 max(H, W); one case with Wo = 130"""
    from data import device_augment as DA
    cases = []
    shapes = (('none', (40, 52, 32, 32)), ('elastic', (40, 52, 32, 32)), ('grid', (36, 60, 30, 130)),
              ('optical', (52, 40, 32, 32)))
    for ki, (kind, (H, W, Ho, Wo)) in enumerate(shapes):
        n = 4
        ps, gm, fields = [], np.zeros((n, Wo + Ho), np.float32), np.zeros((n + 1, Ho, Wo, 2), np.float32)
        for i in range(n):
            for grow in (1.3, 1.6, 2.0, 2.5, 3.2):     # the smallest window that puts 25 % of the points outside
                rng = np.random.default_rng([202, ki, i])
                a = _host_affine(rng, Wo, Ho, H, W, grow)
                border, field = i % 2, (i * 3 + 2) % (n + 1)   # fields 2, 0, 3, 1: neither the sample index nor a count
                if kind == 'elastic':
                    c, sq = Wo // 2, min(Ho, Wo) // 3
                    pts1 = np.float32([[c + sq, c + sq], [c + sq, c - sq], [c - sq, c - sq]])
                    pts2 = pts1 + rng.uniform(-3.6, 3.6, size=pts1.shape).astype(np.float32)
                    fields[field] = rng.uniform(-3, 3, size=(Ho, Wo, 2))
                    p = wp(a, border, 1, field, DA._affine_inv(DA._affine_from_points(pts1, pts2)))
                elif kind == 'grid':
                    gm[i, :Wo] = DA.grid_axis(Wo, [1 + rng.uniform(-0.3, 0.3) for _ in range(6)], 5)
                    gm[i, Wo:] = DA.grid_axis(Ho, [1 + rng.uniform(-0.3, 0.3) for _ in range(6)], 5)
                    p = wp(a, border, 2)
                elif kind == 'optical':
                    p = wp(a, border, 3, k=rng.uniform(-1, 1), cx=Wo * 0.5 + round(rng.uniform(-0.5, 0.5)),
                           cy=Ho * 0.5 + round(rng.uniform(-0.5, 0.5)), fx=Wo, fy=Ho)
                else:
                    p = wp(a, border)
                qx, qy = R.distort(p, None, gm[i], fields[field], out_hw=(Ho, Wo))
                sx, sy = p['a'][0] * qx + p['a'][1] * qy + p['a'][2], p['a'][3] * qx + p['a'][4] * qy + p['a'][5]
                if ((sx < 0) | (sx > W - 1) | (sy < 0) | (sy > H - 1)).mean() >= 0.25:
                    break
            ps.append(p)
        cases.append(_case(f'general {kind}', _image(np.random.default_rng([203, ki]), n, H, W), ps, Ho, Wo, Cm=2,
                           gmaps=gm, fields=fields, exact=False))
    return cases


def warp_expected(case, mut=()):
    """Per sample: fp64 levels, the rule's decision for the image, the mask's levels and candidate values, the outside
    share.  mut: oracle mutations, or 'field_by_n' / 'gmap_shift' (per-sample records read at the wrong index)."""
    out = []
    n = len(case['params'])
    Ho, Wo = case['Ho'], case['Wo']
    for i, p in enumerate(case['params']):
        g = case['gmaps'][(i + 1) % n if 'gmap_shift' in mut else i]
        fld = case['fields'][min(i, len(case['fields']) - 1) if 'field_by_n' in mut else p['field']]
        mk = case['mask'][i] if case['mask'] is not None else None
        kw = dict(out_hw=(Ho, Wo), details=True)
        o64, m64, d64 = R.warp(case['img'][i], mk, p, None, g, fld, mut=mut, **kw)
        o32, _, d32 = R.warp(case['img'][i], mk, p, None, g, fld, dtype=np.float32, mut=mut, **kw)
        dec = decide(d64['rounds'], d32['rounds'], o64.shape, not mut)
        H, W = case['img'].shape[1:3]
        sx, sy = d64['sx'], d64['sy']
        rec = dict(img=o64, dec=dec, pre64=d64['rounds'][0][1], pre32=d32['rounds'][0][1], sx=sx, sy=sy,
                   sx32=d32['sx'], sy32=d32['sy'],
                   outside=float(((sx < 0) | (sx > W - 1) | (sy < 0) | (sy > H - 1)).mean()),
                   coord=float(max(np.abs(sx).max(), np.abs(sy).max())) / max(H, W))
        if mk is not None:
            ex = MARGIN * float(np.abs(d32['sx'].astype(np.float64) - sx).max())
            ey = MARGIN * float(np.abs(d32['sy'].astype(np.float64) - sy).max())
            dx, x_lo, x_hi = boundary(sx, 'rint', False)
            dy, y_lo, y_hi = boundary(sy, 'rint', False)
            ux, uy = dx < ex, dy < ey
            cands = []
            for cx in (x_lo, x_hi):
                for cy in (y_lo, y_hi):
                    mx = np.where(ux, cx, np.rint(sx)).astype(np.int64)
                    my = np.where(uy, cy, np.rint(sy)).astype(np.int64)
                    cands.append(R.mask_at(mk, mx, my, p['border']))
            rec.update(mask=np.rint(m64 * 255.0), mask_und=ux | uy, mask_cands=cands, mask_eps=(ex, ey),
                       mask_dist=np.minimum(np.where(ux, dx, np.inf), np.where(uy, dy, np.inf)))
        out.append(rec)
    return out


def check_warp(case, exp, got_img, got_mask, what=''):
    """got_img [n,Ho,Wo,3] levels, got_mask [n,Cm,Ho,Wo] fp32 in [0, 1] (or None) against warp_expected.  Returns
    (worst observed / eps, largest undecided image share, largest undecided mask share)."""
    ratio = share_i = share_m = 0.0
    for i, e in enumerate(exp):
        w = f'{case["name"]} {what} sample {i}'
        if case['exact_image']:
            assert not e['dec']['und'].any() and np.array_equal(np.asarray(got_img[i], np.float64), e['img']), w
        else:
            r, s = check_levels(got_img[i], e['img'], e['dec'], CAP_IMAGE, w)
            ratio, share_i = max(ratio, r), max(share_i, s)
        if got_mask is None or 'mask' not in e:
            continue
        g = np.asarray(got_mask[i])
        assert g.dtype == np.float32
        und = e['mask_und']
        s = float(und.mean())
        assert s <= CAP_MASK, f'{w}: {s:.5f} of the mask undecided'
        assert not (case['exact'] and und.any()), w
        ref = to_float(e['mask'])
        assert np.array_equal(g[:, ~und], ref[:, ~und]), f'{w}: decided mask pixels differ'
        hit = np.zeros(und.shape, bool)
        for c in e['mask_cands']:
            hit |= (g == to_float(c)).all(0)
        assert hit[und].all(), f'{w}: an undecided mask pixel holds neither candidate'
        diff = (g != ref).any(0) & und
        if diff.any():
            ratio = max(ratio, float((e['mask_dist'] / max(max(e['mask_eps']), 1e-300))[diff].max()))
        share_m = max(share_m, s)
    return ratio, share_i, share_m


# ---- colour ----------------------------------------------------------------------------------------------------------
def color_lattice():
    """every (r, g, b) with each channel in range(0, 256, 5) (which ends at 255): 52^3 = 140608 pixels as one
    52 x 2704 image; includes every equal-channel sector boundary of the HSV conversion"""
    v = np.arange(0, 256, 5, dtype=np.float32)
    assert v[-1] == 255
    return np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(len(v), len(v) * len(v), 3)


def _production_color(rng):
    return dict(bc=1, alpha=float(np.float32(1 + rng.uniform(-0.2, 0.2))), beta=float(np.float32(rng.uniform(-0.2, 0.2))))


def color_records():
    """(name, record, exact by construction)"""
    rng = np.random.default_rng(303)
    f32 = lambda v: [float(np.float32(t)) for t in v]      # noqa: E731
    recs = [
        ('bc dyadic up', dict(bc=1, alpha=1.25, beta=0.125), True),
        ('bc dyadic down', dict(bc=1, alpha=0.5, beta=-0.25), True),
        ('bc clips both ends', dict(bc=1, alpha=float(np.float32(2.617)), beta=float(np.float32(-0.613))), False),
        ('gray', dict(gray=1), True),
        ('all off', dict(), True),
        ('bc then gray', dict(bc=1, alpha=float(np.float32(1.1337)), beta=float(np.float32(-0.0713)), gray=1), False),
        ('rgb integer', dict(rgb=1, shift=[3.0, -7.0, 0.0]), True),
        ('rgb half-integer', dict(rgb=1, shift=[2.5, -3.5, 0.5]), True),
        ('rgb clips', dict(rgb=1, shift=[200.25, -180.5, 77.0]), True),
        ('hsv hue below 0', dict(hsv=1, hsv_shift=[-30.0, 0.0, 0.0]), False),
        ('hsv hue past 180, half-integer', dict(hsv=1, hsv_shift=[170.5, 2.0, -3.0]), False),
        ('hsv hue lands on 180', dict(hsv=1, hsv_shift=[90.0, 0.5, 0.0]), False),
        ('hsv hue lands on 0', dict(hsv=1, hsv_shift=[-90.0, 0.0, 1.5]), False),
        ('hsv sat up, val down, clipping', dict(hsv=1, hsv_shift=[0.0, 60.0, -100.0]), False),
        ('hsv sat down, val up, clipping', dict(hsv=1, hsv_shift=[0.0, -60.0, 100.0]), False),
    ]
    for i in range(3):
        p = _production_color(rng)
        if i == 0:
            p.update(rgb=1, shift=f32(rng.uniform(-10, 10, 3)))
        else:
            p.update(hsv=1, hsv_shift=f32([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-1, 1)]), gray=i - 1)
        recs.append((f'production {i}', p, False))
    return recs


def color_big():
    """513 x 512 pixels, one row past the 1024 x 256 threads of the colour kernel's grid; values follow the pixel index"""
    i = np.arange(513 * 512, dtype=np.int64)
    img = np.stack([i % 256, (i // 256 + i // 7) % 256, (i * 7 + i // 65536) % 256], -1).astype(np.float32)
    rng = np.random.default_rng(304)
    p = _production_color(rng)
    p.update(hsv=1, hsv_shift=[float(np.float32(v)) for v in (-8.3, 7.1, 0.6)])
    return img.reshape(513, 512, 3), p


def color_expected(img, p, mut=()):
    o64, d64 = R.color(img, p, details=True, mut=mut)
    o32, d32 = R.color(img, p, dtype=np.float32, details=True, mut=mut)
    return dict(img=o64, img32=o32, dec=decide(d64['rounds'], d32['rounds'], o64.shape, not mut), r64=d64['rounds'],
                r32=d32['rounds'])


def check_color(got, e, exact, what):
    if exact:
        assert not e['dec']['und'].any(), what
        assert np.array_equal(np.asarray(got, np.float64), e['img']), f'{what}: not equal'
        return 0.0, 0.0
    return check_levels(got, e['img'], e['dec'], CAP_IMAGE, what)


# ---- blur ------------------------------------------------------------------------------------------------------------
WMAX = 64
BLUR_SHAPES = ((1, 1, 1), (2, 2, 2), (5, 127, 3), (1, 128, 4), (2, 129, 1), (5, 257, 2), (5, 2, 3), (1, 257, 3))
ASYM = [0.25, 1.0, 0.5]      # asymmetric (reversed taps show), sum 1.75 as the elastic taps carry sqrt(alpha): a
#                              skipped pass shows even where every tap reads the same pixel (H == 1)


def blur_cases():
    """H x W x C over BLUR_SHAPES, sym x round8, per-sample radii in one batch.  'dyadic': integer images with cv2's
    fixed tables (ksize 3 / 5 / 7) and one asymmetric dyadic table -- exact, the .5 ties included.  'gauss': radii
    0, 1, 3, 31 (63 of WMAX = 64 taps; several periods wider than W = 2, H = 1, H = 5) with Gaussian taps."""
    from data import device_augment as DA
    rng = np.random.default_rng(404)
    cases = []
    for sym in (0, 1):
        for round8 in (0, 1):
            for H, W, C in BLUR_SHAPES:
                for taps in ('dyadic', 'gauss'):
                    radius = np.array([0, 1, 2, 3, 1] if taps == 'dyadic' else [0, 1, 3, 31], np.int32)
                    n = len(radius)
                    w = np.zeros((n, WMAX), np.float32)
                    for i, r in enumerate(radius):
                        if r:
                            w[i, :2 * r + 1] = (DA.cv2_gaussian_taps(2 * r + 1) if taps == 'dyadic' else
                                                DA.scipy_gaussian_taps(max(r / 4.0, 0.4))[:2 * r + 1] if sym else
                                                DA.cv2_gaussian_taps(2 * r + 1) if r > 3 else
                                                DA.scipy_gaussian_taps(0.7 * r)[:2 * r + 1])
                    if taps == 'dyadic':
                        w[4, :3] = ASYM
                    ints = taps == 'dyadic' or round8
                    x = (rng.integers(0, 256, size=(n, H, W, C)) if ints else rng.uniform(-1, 1, size=(n, H, W, C)))
                    cases.append(dict(name=f'{taps} {H}x{W}x{C} sym={sym} round8={round8}', x=x.astype(np.float32),
                                      radius=radius, weights=w, sym=sym, round8=round8, exact=taps == 'dyadic'))
    return cases


def blur_expected(case, mut=()):
    out = []
    for i, r in enumerate(case['radius']):
        kw = dict(sym=bool(case['sym']), round8=bool(case['round8']), details=True, mut=mut)
        o64, d64 = R.blur(case['x'][i], int(r), case['weights'][i], **kw)
        o32, d32 = R.blur(case['x'][i], int(r), case['weights'][i], dtype=np.float32, **kw)
        out.append(dict(out=o64, out32=o32, dec=decide(d64['rounds'], d32['rounds'], o64.shape, not mut), pre64=d64.get('pre'),
                        pre32=d32.get('pre')))
    return out


def check_blur(case, exp, got, what=''):
    """returns (worst observed / eps, largest undecided share)"""
    ratio = share = 0.0
    for i, e in enumerate(exp):
        w = f'{case["name"]} {what} sample {i} (radius {case["radius"][i]})'
        g = np.asarray(got[i], np.float64)
        if case['exact'] or case['radius'][i] == 0:
            assert np.array_equal(g, e['out']), f'{w}: not equal'
        elif case['round8']:
            r, s = check_levels(g, e['out'], e['dec'], CAP_IMAGE, w)
            ratio, share = max(ratio, r), max(share, s)
        else:
            ratio = max(ratio, check_close(g, e['out'], e['out32'], w))
    return ratio, share


# ---- ISO noise / ToFloat -----------------------------------------------------------------------------------------------
def iso_cases():
    """(name, images [n,H,W,3] on the uint8 grid, records, seed).  HW = 1; 131072 = 512 x 256 threads exactly; 363 x 362
    = 131406, a second grid-stride round with a tail."""
    rng = np.random.default_rng(505)
    rnd = lambda n, H, W: rng.integers(0, 256, size=(n, H, W, 3)).astype(np.float32)      # noqa: E731
    four = [dict(), dict(iso=1, iso_color_std=0.0, iso_intensity=0.0), dict(iso=1, iso_color_std=0.0, iso_intensity=0.3),
            dict(iso=1, iso_color_std=float(np.float32(9.0)), iso_intensity=float(np.float32(0.45)))]
    H, W = 363, 362
    edge = rnd(4, H, W)
    edge[0] = np.float32([90, 140, 200])                                  # constant: lambda == 0, every count 0
    edge[1] = np.where(rng.random((H, W, 1)) < 0.5, rng.integers(0, 40, (H, W, 3)), rng.integers(215, 256, (H, W, 3)))
    edge[2, :40] = 0                                                       # pure black and pure white: 1 - l == 0
    edge[2, 40:80] = 255
    recs = [dict(iso=1, iso_color_std=0.0, iso_intensity=0.5), dict(iso=1, iso_color_std=5.0, iso_intensity=1.0),
            dict(iso=1, iso_color_std=0.0, iso_intensity=0.25), four[3]]
    return [('HW=1', rnd(4, 1, 1), four, 77), ('HW=131072', rnd(4, 256, 512), four, 2 ** 62 - 1),
            ('HW=363x362', edge, recs, 0x0123456789ABCDEF)]


def _hue_normal(u, dtype):
    """sqrtf(-2 logf(u1)) cosf(6.2831853f u2) from the fp32 uniforms, every operation in dtype"""
    f = np.dtype(dtype).type
    u1, u2 = u[..., 0].astype(dtype), u[..., 1].astype(dtype)
    ang = (np.float32(6.2831853) * u[..., 1]).astype(dtype) if dtype == np.float64 else f(6.2831853) * u2
    return np.sqrt(f(-2) * np.log(u1)) * np.cos(ang)


def iso_expected(case, mut=(), **philox_mut):
    """Per sample: the fp64 levels [H,W,3] with the host-predicted hue noise and Poisson counts, the rule's decision,
    the levels at the smallest and the largest admissible count of every pixel, the luminance sums and lambda."""
    import philox_ref as P
    name, img, recs, seed = case
    n, H, W, _ = img.shape
    HW = H * W
    u = P.iso_uniforms(n, HW, seed, **philox_mut).reshape(n, H, W, 3)
    out = []
    for i, p in enumerate(recs):
        if not p.get('iso'):
            out.append(dict(levels=img[i].astype(np.float64), off=True))
            continue
        s1, s2 = R.lum_stats(img[i])
        lam64, lam32 = R.iso_lambda(s1, s2, HW, p['iso_intensity']), R.iso_lambda(s1, s2, HW, p['iso_intensity'], np.float32)
        c64, p64 = R.poisson(lam64, u[i, ..., 2], details=True)
        c32, p32 = R.poisson(lam32, u[i, ..., 2], dtype=np.float32, details=True)
        assert p64['K'] == p32['K'], name
        K, F, u3 = p64['K'], p64['F'], u[i, ..., 2].astype(np.float64)
        eps_f = MARGIN * float(np.abs(p32['F'].astype(np.float64) - F).max())
        # the counts whose CDF step lies within eps of u: one count where decided, two next to a step, more only in
        # the far tail, where the steps are closer together than eps
        c_lo = np.minimum(np.searchsorted(F, u3 - eps_f, side='left'), K).astype(np.float64)
        c_hi = np.minimum(np.searchsorted(F, u3 + eps_f, side='left'), K).astype(np.float64)
        und_c = c_lo != c_hi
        assert ((c_lo <= c64) & (c64 <= c_hi) & (c_lo <= c32) & (c32 <= c_hi)).all(), name
        if 'poisson_off_by_one' in mut:
            c64 = c64 + 1
        hue64 = _hue_normal(u[i], np.float64) * np.float64(p['iso_color_std'])
        hue32 = _hue_normal(u[i], np.float32) * np.float32(p['iso_color_std'])
        _, d64 = R.iso_finish(img[i], p, hue64, c64, details=True)
        _, d32 = R.iso_finish(img[i], p, hue32, c64, dtype=np.float32, details=True)
        dec = decide(d64['rounds'], d32['rounds'], d64['levels'].shape)
        alts = [R.iso_finish(img[i], p, hue64, c, details=True)[1]['levels'] for c in (c_lo, c_hi)]
        out.append(dict(levels=d64['levels'], dec=dec, alts=alts, und_count=und_c, counts=c64, c_lo=c_lo, c_hi=c_hi,
                        lam=float(lam64), lam32=float(lam32), stats=(s1, s2), eps_f=eps_f, off=False, F=F, K=K))
    return out


def check_iso(case, exp, got, stats=None, what=''):
    """got [n,3,H,W] fp32 in [0, 1] and the fp64 sums [n,2] against iso_expected.  Every value must be a ToFloat level
    bit for bit.  The ISO image has no cap on its undecided share: without luminance noise the HLS round trip is the
    identity, so every value lands within rounding of an integer before the floor, in fp64 as in fp32; the two-sided
    rule (the level below the integer or the integer itself) is what holds there.  Returns (worst observed / eps, largest
    undecided share of the image, largest undecided share of the counts, worst sums error / bound)."""
    name, img, recs, _ = case
    ratio = share = share_c = rstat = 0.0
    HW = img.shape[1] * img.shape[2]
    for i, e in enumerate(exp):
        w = f'{name} {what} sample {i}'
        g = np.asarray(got[i])
        assert g.dtype == np.float32
        lv = np.rint(g.astype(np.float64) * 255.0)
        assert np.array_equal(to_float(lv), g), f'{w}: not ToFloat levels'
        lv = lv.transpose(1, 2, 0)
        if e['off']:
            assert np.array_equal(lv, e['levels']), f'{w}: ToFloat alone differs'
            continue
        sc = float(e['und_count'].mean())
        assert sc <= CAP_POISSON, f'{w}: {sc:.5f} of the Poisson counts undecided'
        share_c = max(share_c, sc)
        uc = e['und_count'][..., None] & np.ones(3, bool)
        dec = dict(e['dec'], und=e['dec']['und'] & ~uc)
        keep = np.where(uc, e['levels'], lv)                      # the pixels with an undecided count go separately
        r, s = check_levels(keep, e['levels'], dec, 1.0, w)
        ratio, share = max(ratio, r), max(share, float(e['dec']['und'].mean()))
        near = (lv >= e['alts'][0] - 1.0) & (lv <= e['alts'][1] + 1.0)     # the levels grow with the count
        assert near[uc].all(), f'{w}: a pixel with an undecided count lies outside its admissible counts'
        if stats is not None:
            for j in range(2):
                bound = HW * 2.0 ** -53 * e['stats'][j]
                err = abs(float(stats[i][j]) - e['stats'][j])
                assert err <= bound, f'{w}: luminance sum {j} off by {err:.3e} (bound {bound:.3e})'
                rstat = max(rstat, err / bound if bound > 0 else 0.0)
    return ratio, share, share_c, rstat


# ---- composition -----------------------------------------------------------------------------------------------------
# DeviceAugment.train / .unsupervised with every stage forced on; S = 130 is two column blocks, 96 x 80 inputs, batch 6;
# both seeds draw at least one elastic sample (tests/test_augment_exact_host.py)
COMPOSITION = dict(S=130, hw=(96, 80), n=6, seeds=(1, 2), kw=dict(distort_p=1.0, blur_p=1.0, iso_p=1.0, color_p=1.0))
