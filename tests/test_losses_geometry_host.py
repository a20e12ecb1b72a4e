"""Host-side proof (no GPU) of the designs in exact_losses.py that test_losses_geometry.py runs on the device.

For every case, on the fp32 CPU form (the fp64 restatement evaluated at float32) and the fp64 form:
  1. the background adds exactly 0 in fp32 (BCE and the binary entropy: below 2^-60 of the total) and below 2^-60 of
     the total in fp64;
  2. every probe weighs at least 100 x (rtol |total| + atol) of the bound used on the device, so a missing or doubled
     probe cannot pass (see exact_losses.PROBE_FACTOR for the three families whose per-element term is bounded and
     cannot reach 100 under a mean over 262,144 elements), and the probes' contributions are pairwise 1 % apart;
  3. the fp32 CPU result itself meets the device bound against fp64: the reference alone stays inside the bound;
  4. OHEM: the fp64 group gaps hold and the expected counts equal ohem_state64's;
  5. each shape does cross the launch threshold it is there for.
"""
import numpy as np
import pytest
import torch

import exact_losses as E
from test_hip_losses_ext import GRAD_TOL, LOSS_TOL

F32 = torch.float32


def close(a, ref, tol):
    return bool(np.allclose(a, ref, equal_nan=True, **tol))


def _maxabs(a):
    """largest finite |a| (NaN when nothing is finite)"""
    a = np.abs(np.asarray(a, np.float64)).reshape(-1)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else float('nan')


def check_fp32_meets_the_bound(case):
    l64, g64, w = E.ref64(case)
    l32, g32 = E.evaluate(case, F32, w)
    print(f'{case.name}: loss fp32-fp64 {_maxabs(l32 - l64):.3e} (max |loss| {_maxabs(l64):.3e}); grad fp32-fp64 '
          f'{_maxabs(g32 - g64):.3e} (max |grad| {_maxabs(g64):.3e})')
    assert np.array_equal(np.isnan(l32), np.isnan(l64)) and np.array_equal(np.isnan(g32), np.isnan(g64))
    assert close(l32, l64, LOSS_TOL)
    assert close(g32, g64, GRAD_TOL)
    assert np.all(g32[g64 == 0] == 0)


@pytest.mark.parametrize('name', E.PROBE_CASES)
def test_probe_design(name):
    case = E.probe_case(name)
    l64, g64, _ = E.ref64(case)
    total = float(np.abs(l64).max())
    assert len(case.sites) <= 16 and E.crosses(case)                                        # 5
    # 1. the background
    b32, b64 = np.abs(E.background(case, F32)).max(), np.abs(E.background(case, E.F64)).max()
    print(f'{name}: total {total:.6e}  background fp32 {b32:.3e} fp64 {b64:.3e}')
    if case.family in ('bce_mean', 'bce_sum', 'bce_none', 'bent'):
        assert b32 <= E.PAD * total
    else:
        assert b32 == 0
    assert b64 <= E.PAD * total
    # 2. the weight of every probe
    if case.family not in ('ce_none', 'bce_none'):          # per-element outputs: every element is compared itself
        con = np.abs(E.contributions(case))
        con = con[:len(con) - case.kw.get('ignored', 0)]    # ignore-labelled probes weigh nothing, by design
        bound = LOSS_TOL['rtol'] * total + LOSS_TOL['atol']
        print(f'{name}: smallest probe / bound = {con.min() / bound:.1f} (asked: {E.probe_factor(case)})')
        assert con.min() >= E.probe_factor(case) * bound
        if case.family != 'dice':                           # integer counts: equal probes are meant there
            assert E._distinct(con)
    # 3. the reference alone stays within the bound
    check_fp32_meets_the_bound(case)
    assert np.abs(g64).max() > 0 or case.family == 'dice'


def test_probe_positions():
    """every position of the list that fits is probed, with the sample boundary"""
    for name in E.PROBE_CASES:
        case = E.probe_case(name)
        if case.edge != 'red':
            continue
        flat = case.family in E.FLAT
        n = case.x.size if flat else case.npix
        per = n // case.x.shape[0]
        got = set()
        for s in case.sites:
            if flat:
                got.add(int(np.ravel_multi_index(s, case.x.shape)))
            else:
                got.add(s[0] * case.hw + int(np.ravel_multi_index(s[2:], case.x.shape[2:])))
        want = {0, 63, 64, 255, 256, 65535, 65536, 262143, 262144, 262145, n - 1}
        if case.x.shape[0] > 1:
            want |= {per - 1, per}
        assert got == want, name
    nfl = E.probe_case('nfl_plane')
    hw = nfl.hw
    offs = {(s[0] * 3 + s[1], s[2] * 131 + s[3]) for s in nfl.sites}
    for pl in (0, 5):
        assert {(pl, 16383), (pl, 16384), (pl, 16385), (pl, hw - 1)} <= offs
    assert (3, 0) in offs and (0, 0) in offs
    for name, per in (('dice_plane', 131 * 131), ('dicep_sample', 2 * 95 * 97), ('logdicep_sample', 2 * 95 * 97)):
        case = E.probe_case(name)
        offs = {(s[0], int(np.ravel_multi_index(s[-2:] if name == 'dice_plane' else s[1:],
                                                 case.x.shape[-2:] if name == 'dice_plane' else case.x.shape[1:])))
                for s in case.sites}
        for b in (0, 1):
            assert {(b, 16383), (b, 16384), (b, 16385), (b, per - 1)} <= offs, name


def test_dice_design_is_integer_valued():
    case = E.probe_case('dice_plane')
    x, t = torch.from_numpy(np.array(case.x)), torch.from_numpy(np.array(case.t))
    p = torch.softmax(x, 1)
    assert set(np.unique(p.numpy())) == {0.0, 1.0}                     # exactly one-hot in fp32
    T, P, I = t.sum((2, 3)), p.sum((2, 3)), (p * t).sum((2, 3))        # noqa: E741
    assert bool((T[:, 1:] >= 2).all()) and bool((T[:, 1:] < 10).all()) and bool((P[:, 1:] < 10).all())
    assert bool((I[:, 1:] < T[:, 1:]).any()) and bool((I[:, 1:] > 0).any())    # partly on the wrong class


def test_consistency_counts():
    for name in ('cons_red', 'cons_batch', 'cons_quiet_red', 'cons_quiet_batch'):
        case = E.probe_case(name)
        for dtype in (F32, E.F64):
            _, frac, cnt = E.consistency64(E._tt(case.x, dtype), E._tt(case.t, dtype), E.CONS_THR)
            assert cnt == case.kw['count']
        kinds = case.kw['kinds']
        assert 0 < sum(kinds) < len(kinds)                              # both kinds of probe
        assert np.float32(cnt / case.npix) == np.float32(float(frac))


@pytest.mark.parametrize('family', E.SWEEP_FAMILIES)
def test_sweep_design(family):
    assert set(E.WIDTHS) >= {1, 2, 4, 8, 16, 32, 64} and set(E.WIDTHS) >= {3, 5, 9, 17, 33}
    for hw in E.SWEEP_HW:
        assert (2 * hw[0] * hw[1] < 256) == (hw == (7, 9)) and (hw[0] * hw[1]) % 64 != 0
        for C in E.WIDTHS:
            case = E.sweep_case(family, C, hw)
            assert case.x.shape == (2, C) + hw and E.crosses(case)
            check_fp32_meets_the_bound(case)


@pytest.mark.parametrize('family', E.GRID_FAMILIES)
def test_grid_design(family):
    case = E.grid_case(family)
    assert E.crosses(case) and case.npix == 1_048_869
    check_fp32_meets_the_bound(case)
    if family == 'ohem':    # the selection does not hang on fp32 rounding: no pred within 1e-6 of the threshold
        thr, sel = E.ohem_state64(E._tt(case.x, E.F64), E._tt(case.t, E.F64), case.kw['thres'], case.kw['min_kept'])
        p = torch.softmax(E._tt(case.x, E.F64), 1).gather(1, E._tt(case.t, E.F64).argmax(1, keepdim=True))
        assert thr == case.kw['thres'] and float((p - thr).abs().min()) > 1e-6 and 0 < int(sel.sum()) < case.npix
    if family == 'cons':
        gap = (torch.sigmoid(E._tt(case.t, E.F64)) - E.CONS_THR).abs().min()
        assert float(gap) > 1e-3


def test_smooth_labels_reference_is_exact_in_fp32():
    t = torch.from_numpy(np.array(E.grid_case('ce').t))
    ref = t * (1 - 0.1) + 0.1 / t.size(1)
    assert np.allclose(ref.numpy(), E.smooth64(t.double(), 0.1).numpy(), rtol=1e-6, atol=0)
    assert t.numel() > E.GRID_SPAN and t.numel() % 256 != 0


# ---- 4. the OHEM selection design --------------------------------------------------------------------------------
def _key(p):
    return int(np.float32(p).view(np.uint32))


def test_ohem_design_gaps_and_keys():
    d = E.ohem_design()
    assert sorted(d.sizes)[:3] == [1, 2, 3] and {255, 256, 257} <= set(d.sizes) and max(d.sizes) > 65536
    assert d.cum[-1] < d.npix - 1 and len(d.pred) == 12
    # fp32 preds as the CPU computes them from the very logits
    p32 = [float(torch.softmax(torch.tensor([0.0, a], dtype=F32), 0)[0]) for a in d.a]
    gaps = np.diff(d.pred)
    close_pairs = [i for i, g in enumerate(gaps) if g < 1e-3]
    assert len(close_pairs) == 1
    i = close_pairs[0]
    ulp = float(np.spacing(np.float32(d.pred[i])))
    print(f'close pair: {d.pred[i]!r} {d.pred[i + 1]!r} gap {gaps[i]:.3e} = {gaps[i] / ulp:.0f} ulp; keys '
          f'{_key(p32[i]):#x} {_key(p32[i + 1]):#x}')
    assert 100 * ulp <= gaps[i] < 2e-6
    assert _key(p32[i]) >> 8 == _key(p32[i + 1]) >> 8 and _key(p32[i]) != _key(p32[i + 1])
    # room for a few ulp of difference between this CPU's expf and the device's
    assert 8 <= _key(p32[i]) & 255 and _key(p32[i + 1]) & 255 <= 247
    assert {d.sizes[i], d.sizes[i + 1]} == {256, 257}
    assert d.pred[0] < 2.0 ** -20 and all(abs(a - b) < 1e-6 for a, b in zip(p32, d.pred))
    # the background's pred is exactly 1.0 in fp32
    bg = torch.softmax(torch.tensor([30.0, -30.0]), 0)[0]
    assert float(bg) == 1.0
    lo, mid, hi = d.thresholds
    assert lo < d.pred[0] and d.pred[5] + 1e-3 < mid < d.pred[6] - 1e-3 and d.pred[-2] < hi < d.pred[-1]


def test_ohem_design_expected_counts():
    d = E.ohem_design()
    ks = d.ranks()
    assert {1, d.npix - 1, 10 * d.npix} <= set(ks) and all(c in ks and c - 1 in ks for c in d.cum)
    x, t = E._tt(d.x, E.F64), E._tt(d.t, E.F64)
    ce = E.ce64(x, t, 'none')
    for thres in d.thresholds:
        for k in ks:
            thr, sel = E.ohem_state64(x, t, thres, k)
            e_thr, e_kept, e_loss = d.expected(k, thres)
            assert int(sel.sum()) == e_kept, (k, thres)
            assert abs(thr - e_thr) < 1e-12
            loss = float(ce[sel].mean())
            assert (np.isnan(loss) and np.isnan(e_loss)) or abs(loss - e_loss) <= 1e-12 * abs(e_loss)
    # the regimes are all there: the threshold is thres / an order statistic; the statistic sits inside a tie group,
    # on its first and on its last element; nothing is kept
    kept = {(k, th): d.expected(k, th)[1] for th in d.thresholds for k in ks}
    assert 0 in kept.values() and d.cum[-1] in kept.values() and len(set(kept.values())) >= len(d.sizes)
