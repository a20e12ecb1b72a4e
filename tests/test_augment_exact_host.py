"""CPU-only checks of the per-pixel augmentation tests (tests/test_augment_exact.py): the conditions of the rule hold on
the oracle alone (undecided-share caps, the outside share of the general warp cases, exactness of the cases that are
exact by construction), the oracle's helpers have known answers, and the comparators of tests/augment_cases.py accept
the oracle and reject a reference with each of the listed mistakes on the very case tables the device test uses."""
import math

import numpy as np
import pytest

import augment_cases as A
import philox_ref as P
from oracle import augment_ref as R


# ---- known answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 2, 3, 5, 8))
def test_reflect_against_mirror_tiling(n):
    """reflect-101 (... c b | a b c | b a ...) and scipy 'reflect' (... b a | a b c | c b ...) against tiled arrays"""
    reps, base = 12, np.arange(n)
    t101 = np.concatenate([base, base[-2:0:-1]]) if n > 1 else base      # one period; tiled both ways from index 0
    tsym = np.concatenate([base, base[::-1]])
    i = np.arange(-4 * len(tsym), 4 * len(tsym) + 3)
    t = np.tile(t101, 2 * reps * 4)
    assert R.reflect101(i, n).tolist() == [int(t[k + reps * 4 * len(t101)]) for k in i]
    t = np.tile(tsym, 2 * reps)
    assert R.reflect_sym(i, n).tolist() == [int(t[k + reps * len(tsym)]) for k in i]


@pytest.mark.parametrize('lam', (0.0, 0.5, 3.0, 17.4, 80.0))
def test_poisson_against_cdf_sums(lam):
    """the count is the number of CDF values below u, the CDF summed in fp64 from exp(-lam + k log lam - lgamma(k + 1));
    uniforms closer than 1e-9 to a step are left out"""
    u = P.u01(P.philox(P.counters(0, 4096), 3, P.WORD3_ISO, 11)[:, 2])
    pmf = [math.exp(-lam + (k * math.log(lam) if lam > 0 else 0.0) - math.lgamma(k + 1)) if lam > 0 or k == 0 else 0.0
           for k in range(400)]
    cdf = np.array([math.fsum(pmf[:k + 1]) for k in range(400)])
    want = (u.astype(np.float64)[:, None] > cdf[None, :]).sum(1)
    clear = np.abs(u.astype(np.float64)[:, None] - cdf[None, :]).min(1) > 1e-9
    got, det = R.poisson(lam, u, details=True)
    assert clear.mean() > 0.99 and np.array_equal(got[clear], want[clear].astype(np.float64))
    assert abs(float(got.mean()) - lam) <= 5 * math.sqrt(max(lam, 1e-12) / 4096) + 1e-12
    if lam == 0:
        assert (got == 0).all() and det['F'].tolist() == [1.0, 1.0]
    got32 = R.poisson(lam, u, dtype=np.float32)
    assert got32.dtype == np.float32 and float(np.abs(got32 - got).max()) <= 1


def test_lum_stats_and_lambda():
    img = np.float32([[[0, 0, 0], [255, 255, 255]], [[10, 200, 30], [255, 0, 0]]])
    l = [0.0, 1.0, 0.5 * (float(np.float32(200) / np.float32(255)) + float(np.float32(10) / np.float32(255))), 0.5]
    s1, s2 = R.lum_stats(img)
    assert s1 == math.fsum(l) and abs(s2 - math.fsum(v * v for v in l)) < 1e-15
    var = s2 / 4 - (s1 / 4) ** 2
    assert R.iso_lambda(s1, s2, 4, 0.25) == math.sqrt(var) * 0.25 * 255
    assert R.iso_lambda(s1, s2, 4, 1.0) == 80 and R.iso_lambda(4.0, 4.0, 4, 1.0) == 0
    assert R.iso_lambda(s1, s2, 4, 0.25, np.float32).dtype == np.float32


def test_dtype_keyword_keeps_the_default_results():
    """fp64 is the default and what the oracle always returned; fp32 only changes the arithmetic"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    p = A.wp([0.7, 0.1, 1.3, -0.1, 0.8, 0.4])
    a, _ = R.warp(img, None, p, 6)
    b, _, det = R.warp(img, None, p, 6, dtype=np.float64, details=True)
    c, _ = R.warp(img, None, p, 6, dtype=np.float32)
    assert np.array_equal(a, b) and a.dtype == np.float64 and c.dtype == np.float32 and np.abs(a - c).max() <= 1
    assert np.array_equal(np.rint(np.clip(det['rounds'][0][1], 0, 255)), a)


# ---- warp ------------------------------------------------------------------------------------------------------------
def _oracle_as_device(exp):
    gi = np.stack([e['img'] for e in exp]).astype(np.float32)
    gm = np.stack([A.to_float(e['mask']) for e in exp]) if 'mask' in exp[0] else None
    return gi, gm


def test_warp_exact_cases_are_exact():
    """fp32 and fp64 restatements agree bit for bit on every coordinate and every pre-rounding sum, nothing is
    undecided; for the optical case this holds for the coordinates (and so the mask), its image goes by the rule"""
    names = []
    for case in A.warp_exact_cases():
        exp = A.warp_expected(case)
        for e in exp:
            assert np.array_equal(e['sx'], e['sx32']) and np.array_equal(e['sy'], e['sy32']), case['name']
            assert not e['mask_und'].any() and e['mask_eps'] == (0.0, 0.0), case['name']
            if case['exact_image']:
                assert np.array_equal(e['pre64'], e['pre32']) and not e['dec']['und'].any(), case['name']
                assert e['dec']['eps']['bilinear'] == 0.0
        A.check_warp(case, exp, *_oracle_as_device(exp))
        names.append(case['name'])
    ties = [e for c in A.warp_exact_cases() if c['name'] == 'decimate' for e in A.warp_expected(c)]
    assert all(((e['pre64'] - np.floor(e['pre64'])) == 0.5).sum() >= 5 for e in ties)                  # exact .5 ties
    assert all((np.abs(e['sx'] - np.floor(e['sx'])) == 0.5).all() for e in ties)                       # mask on k + 0.5
    assert {'identity', 'hflip', 'decimate', 'magnify', 'rot90', 'shear', 'periods', 'H=1', 'W=1'} <= set(names)
    assert {f'Wo={w} Ho={h}' for w in (1, 127, 128, 129, 257) for h in (1, 3)} <= set(names)
    assert {c['mask'].shape[3] for c in A.warp_exact_cases()} >= {1, 2, 3, 5}


def test_warp_general_conditions():
    """caps (asserted inside check_warp), at least 20 % of the sampling points outside the image in every sample,
    |coordinate| <= 8 max(H, W), both borders and all four kinds, one case 130 wide"""
    cases = A.warp_general_cases()
    assert {p['distort'] for c in cases for p in c['params']} == {0, 1, 2, 3}
    assert any(c['Wo'] == 130 for c in cases) and all(max(c['img'].shape[1:3]) <= 96 for c in cases)
    for case in cases:
        assert {p['border'] for p in case['params']} == {0, 1}
        exp = A.warp_expected(case)
        for i, e in enumerate(exp):
            assert e['outside'] >= 0.2 and e['coord'] <= 8, (case['name'], i, e['outside'], e['coord'])
        r, si, sm = A.check_warp(case, exp, *_oracle_as_device(exp))
        print(f'{case["name"]}: undecided share image {si:.4f} (cap {A.CAP_IMAGE}) mask {sm:.5f} (cap {A.CAP_MASK}); eps '
              f'{max(e["dec"]["eps"]["bilinear"] for e in exp):.2e} levels, {max(max(e["mask_eps"]) for e in exp):.2e} px')
        fld = [p['field'] for p in case['params'] if p['distort'] == 1]
        assert fld != sorted(fld) or not fld


WARP_MUTANTS = ('reflect_edge', 'tap_shift', 'swap_lxly', 'trunc', 'half_up', 'nearest_half_up', 'field_by_n',
                'gmap_shift', 'channels', 'border_clamp')


def test_warp_comparator_rejects_mutants():
    tables = {'exact': A.warp_exact_cases(), 'general': A.warp_general_cases()}
    for tname, cases in tables.items():
        exps = [A.warp_expected(c) for c in cases]
        for mut in WARP_MUTANTS:
            hits = [c['name'] for c, e in zip(cases, exps)
                    if A.rejects(A.check_warp, c, e, *_oracle_as_device(A.warp_expected(c, mut=(mut,))))]
            print(f'{tname:8s} {mut:16s} rejected by {len(hits)} of {len(cases)} cases')
            # the two tie rules differ from round-half-even on exact ties alone, which only the exact table holds
            # (under the rule a value on a boundary is undecided)
            assert hits or (tname == 'general' and mut in ('half_up', 'nearest_half_up')), (tname, mut)


# ---- colour ----------------------------------------------------------------------------------------------------------
def test_color_cases_and_mutants():
    lat = A.color_lattice()
    assert lat.shape == (52, 2704, 3) and len(np.unique(lat.reshape(-1, 3), axis=0)) == 52 ** 3
    recs = A.color_records()
    names = [r[0] for r in recs]
    assert names.index('all off') not in (0, len(names) - 1)
    exps = {}
    for name, p, exact in recs:
        e = exps[name] = A.color_expected(lat, p)
        if exact:      # no decision value may be inexact
            assert all(a[1] is None or np.array_equal(a[1], b[1]) for a, b in zip(e['r64'], e['r32'])), name
            assert np.array_equal(e['img'], e['img32'])
        r, s = A.check_color(e['img'].astype(np.float32), e, exact, name)
        print(f'{name}: undecided share {s:.5f} (cap {A.CAP_IMAGE})')
    assert np.array_equal(exps['all off']['img'], lat)
    # the wraps are reached: hue + shift on 0 and on 180, below 0 and past 180; both clips of saturation and value
    for name, lo, hi in (('hsv hue lands on 180', 180, 180), ('hsv hue lands on 0', 0, 0), ('hsv hue below 0', -30, -1),
                         ('hsv hue past 180, half-integer', 180.5, 400)):
        h = dict((a[0], a) for a in exps[name]['r64'])['hsv.h'][3]
        h = np.where(h >= 180, h - 180, h) + {n: q for n, q, _ in recs}[name]['hsv_shift'][0]
        assert ((h >= lo) & (h <= hi)).any(), name
    for name in ('hsv sat up, val down, clipping', 'hsv sat down, val up, clipping'):
        sv = dict((a[0], a) for a in exps[name]['r64'])['hsv.shift_sv'][1]
        assert (sv < 0).any() and (sv > 255).any(), name
    bc = dict((a[0], a) for a in exps['bc clips both ends']['r64'])['bc'][1]
    assert (bc < 0).any() and (bc > 255).any()
    for mut in ('trunc', 'half_up', 'channels', 'hue360'):
        hit = next((name for name, p, exact in recs if (mut != 'hue360' or p.get('hsv')) and A.rejects(
            A.check_color, A.color_expected(lat, p, mut=(mut,))['img'].astype(np.float32), exps[name], exact, name)), None)
        print(f'colour {mut:10s} first rejected by the record {hit!r}')
        assert hit, mut
    img, p = A.color_big()
    assert img.shape[0] * img.shape[1] > 1024 * 256
    e = A.color_expected(img, p)
    print('513 x 512: undecided share %.5f' % A.check_color(e['img'].astype(np.float32), e, False, 'big')[1])
    tail = e['img'].astype(np.float32).copy()
    tail[-1, -1, 0] += 2                                   # the last pixel of the second grid-stride round counts
    assert A.rejects(A.check_color, tail, e, False, 'big')


# ---- blur ------------------------------------------------------------------------------------------------------------
BLUR_MUTANTS = ('reflect_swap', 'tap_shift', 'taps_reversed', 'skip_vert_h1', 'trunc', 'half_up')


def test_blur_cases_and_mutants():
    cases = A.blur_cases()
    assert {c['x'].shape[2] for c in cases} == {1, 2, 127, 128, 129, 257} and {c['x'].shape[1] for c in cases} == {1, 2, 5}
    assert {c['x'].shape[3] for c in cases} == {1, 2, 3, 4} and {(c['sym'], c['round8']) for c in cases} == \
        {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(set(c['radius']) >= {0, 1, 3, 31} for c in cases)
    exps, worst = [], 0.0
    for c in cases:
        exp = A.blur_expected(c)
        if c['exact']:
            assert all(np.array_equal(e['out'], e['out32']) and np.array_equal(e['pre64'], e['pre32']) for e in exp if
                       e['pre64'] is not None), c['name']
        _, s = A.check_blur(c, exp, [e['out'].astype(np.float32) for e in exp])
        worst = max(worst, s)
        exps.append(exp)
    print(f'blur: largest undecided share {worst:.5f} (cap {A.CAP_IMAGE}) over {len(cases)} cases')
    ties = [e for c, exp in zip(cases, exps) if c['exact'] and c['round8'] for e in exp if e['pre64'] is not None]
    assert sum(int((np.abs(e['pre64'] - np.floor(e['pre64'])) == 0.5).sum()) for e in ties) > 10        # exact .5 ties
    for mut in BLUR_MUTANTS:
        for table in ('dyadic', 'gauss'):
            hits = 0
            for c, exp in zip(cases, exps):
                if c['name'].startswith(table):
                    bad = [e['out'].astype(np.float32) for e in A.blur_expected(c, mut=(mut,))]
                    hits += A.rejects(A.check_blur, c, exp, bad)
            print(f'blur {table:6s} {mut:14s} rejected by {hits} cases')
            # Gaussian taps are symmetric; round-half-up differs on exact ties alone, which the rule leaves undecided
            assert hits or (table == 'gauss' and mut in ('taps_reversed', 'half_up')), (mut, table)


# ---- ISO noise / ToFloat -----------------------------------------------------------------------------------------------
def _iso_as_device(exp):
    return np.stack([A.to_float(e['levels']).transpose(2, 0, 1) for e in exp])


def test_iso_cases_and_mutants():
    cases = A.iso_cases()
    assert [c[1].shape[1] * c[1].shape[2] for c in cases] == [1, 131072, 363 * 362] and 363 * 362 > 512 * 256
    for case in cases:
        exp = A.iso_expected(case)
        stats = [e.get('stats', (0.0, 0.0)) for e in exp]
        r, s, sc, _ = A.check_iso(case, exp, _iso_as_device(exp), stats)
        print(f'{case[0]}: undecided share image {s:.4f} (no cap), counts {sc:.6f} (cap {A.CAP_POISSON}); lambda '
              f'{[round(e["lam"], 3) for e in exp if not e["off"]]}')
        if case[0] == 'HW=363x362':
            assert exp[0]['lam'] == 0 and (exp[0]['counts'] == 0).all()                        # constant image
            plain = R.iso_finish(case[1][0], dict(iso=1), details=True)[1]['levels']             # luminance unchanged:
            assert np.array_equal(exp[0]['levels'], plain)                                       # the conversion alone
            assert exp[1]['lam'] == 80 and exp[1]['lam32'] == 80                                 # the clip
            assert (case[1][2] == 0).all(-1).any() and (case[1][2] == 255).all(-1).any()         # 1 - l == 0
            muts = [('count off by one', dict(mut=('poisson_off_by_one',))), ('nine rounds', dict(rounds=9)),
                    ('c3 = 0', dict(word3=0))]
            for name, kw in muts:
                assert A.rejects(A.check_iso, case, exp, _iso_as_device(A.iso_expected(case, **kw))), name
            bad = [(s1 * (1 + 1e-9), s2) for s1, s2 in stats]
            assert A.rejects(A.check_iso, case, exp, _iso_as_device(exp), bad)
            tail = _iso_as_device(exp)
            tail[3, 2, -1, -1] = A.to_float(np.rint(tail[3, 2, -1, -1] * 255) - 3 if tail[3, 2, -1, -1] > 0.5 else 3.0)
            assert A.rejects(A.check_iso, case, exp, tail)


# ---- composition -----------------------------------------------------------------------------------------------------
def test_composition_seeds_draw_every_stage():
    from data import device_augment as DA
    for seed in A.COMPOSITION['seeds']:
        aug = DA.DeviceAugment(A.COMPOSITION['S'], seed=seed, **A.COMPOSITION['kw'])
        warp, color, _, radius, _, nf = aug.draw(A.COMPOSITION['n'], *A.COMPOSITION['hw'], train=True)
        kinds = [w.distort for w in warp]
        assert nf >= 1 and kinds.count(1) == nf and all(k > 0 for k in kinds), (seed, kinds)
        assert (radius > 0).all() and all(c.iso and c.bc for c in color)
        assert any(c.rgb or c.hsv for c in color)
