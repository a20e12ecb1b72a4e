"""Keeps tests/exact_cowmix.py honest without a GPU: every case has the property its row of CASES is there for, the
fma32 restatement of the two passes agrees with the oracle's blur, the designed-statistics facts hold, a host model of
the device passes every stage check, and every stage check rejects the mutation it exists for when the mutant's output
is fed to it as the device result."""
import numpy as np
import pytest

import exact_cowmix as C
from oracle import cowmix_ref

F32 = np.float32
NAMES = [c[0] for c in C.CASES]


def _model(name, variant=None, p=None, mutate=None):
    case = C.CASE_BY_NAME[name]
    return C.device_model(C.noise_of(name, variant), C.sigmas_of(case), C.p_of(case) if p is None else p, mutate)


def test_every_case_has_its_edge():
    for name, (B, H, W), sig in C.CASES:
        assert cowmix_ref.window_size(np.asarray(sig, F32)) == C.EXPECT_K[name], name
        assert len(sig) == B
    # banker's rounding of 3 sigma at the half-integers 1.5, 4.5, 7.5 -> 2, 4, 8.  Half-up gives 2, 5, 8 (K = 5, 11,
    # 17: it differs at 4.5 only), half-down 1, 4, 7 (K = 3, 9, 15: it differs at 1.5 and 7.5): the three cases together
    # tell half-to-even from both
    assert [C.window_half_up(np.asarray([s], F32)) for s in (0.5, 1.5, 2.5)] == [5, 11, 17]
    assert [C.window_half_down(np.asarray([s], F32)) for s in (0.5, 1.5, 2.5)] == [3, 9, 15]
    assert [cowmix_ref.window_size(np.asarray([s], F32)) for s in (0.5, 1.5, 2.5)] == [5, 9, 17]
    for s in (0.5, 1.5, 2.5):
        assert float(F32(s)) * 3 % 1 == 0.5
    # the KC = 128 chunk edge: taps per chunk, and the 8-tap unroll's tail
    chunks = lambda K: [min(C.KC, K - k0) for k0 in range(0, K, C.KC)]  # noqa: E731
    assert chunks(127) == [127] and 127 % 8 == 7
    assert chunks(129) == [128, 1] and chunks(257) == [128, 128, 1]
    assert len(chunks(C.KCAP)) == 8 and chunks(C.KCAP)[-1] == 127
    _, (B, H, W), _ = C.CASE_BY_NAME['kcap']
    assert C.KCAP // 2 > W and C.KCAP // 2 > H          # the image lies inside the padding of every row and column
    _, (B, H, W), _ = C.CASE_BY_NAME['k1-second-sweep']
    assert B * H * W > C.SWEEP and C.tiles(H, W) == ((17, 17), (129, 5))
    _, (B, H, W), sig = C.CASE_BY_NAME['multi-sigma']
    assert (H, W) == (C.VT[0] + 1, C.HT[1] + 1) and max(sig) / min(sig) > 10
    for name in ('ragged-63x255', 'ragged-7x261', 'ragged-129x3'):
        _, (B, H, W), _ = C.CASE_BY_NAME[name]
        assert W % 4 and H % 8 and H % C.VT[0] and W % C.VT[1] and W % C.HT[1]
    assert cowmix_ref.window_size(np.asarray(C.BEYOND[2], F32)) == 1025 > C.KCAP
    _, (B, H, W), sig = C.IMPULSE
    assert cowmix_ref.window_size(np.asarray(sig, F32)) == 19 and (63, 255) in C.IMPULSE_AT and (64, 256) in C.IMPULSE_AT
    lay, total = C.carve(3, 65, 257)
    assert all(o % 16 == 0 for o, _, _ in lay.values()) and total % 16 == 0
    assert lay['taps'][0] == 48 + 16 and lay['tmp'][0] == 64 + C._a16(4 * 1023 * 3)
    with pytest.raises(AssertionError, match='layout'):
        C.decode(np.zeros(total, np.uint8), 3, 65, 257, total + 16)


def test_measured_constants():
    """ERFINV_M is what the docstring records (a correctly rounded fp32 erfinv: under one half ulp relative, i.e. under
    1 x 2^-24, and close to it over 4094 arguments), and the oracle's fp32 taps keep to the recorded error"""
    m = C.erfinv_m()
    print('erfinv rounding, units of 2^-24:', m)
    assert 0.9 < m <= 1.0
    worst = 0.0
    for name, _, sig in C.CASES:
        K = C.EXPECT_K[name]
        for s in sig:
            g64, g32 = C.taps64(K, s), cowmix_ref.gaussian_taps(K, F32(s)).astype(np.float64)
            normal = g64 >= 4 * C.FLT_MIN
            worst = max(worst, float((np.abs(g32 - g64)[normal] / g64[normal]).max()))
            assert abs(g64.sum() - 1) < 1e-15 and (K < 3 or int(np.argmax(g64)) == (K + 1) // 2)
    print('oracle fp32 taps, worst relative error over the normal-range taps:', worst)
    assert worst < 4e-7


@pytest.mark.parametrize('name', ['half-1.5', 'multi-sigma', 'ragged-7x261'])
def test_fma_blur_against_the_oracle_and_fp64(name):
    """blur_restate on the oracle's taps against the oracle's blur_field (a product and a sum where the kernel has one
    fma: a few ulp of the accumulated magnitude apart) and against the same sum in fp64"""
    case = C.CASE_BY_NAME[name]
    noise, sig = C.noise_of(name), C.sigmas_of(case)
    run = _model(name)
    ref = cowmix_ref.blur_field(np.array(noise), sig)
    K = run['K']
    mag = C.blur_restate(C.blur_restate(np.abs(noise), run['taps'], K, 1), run['taps'], K, 2).astype(np.float64)
    assert (np.abs(run['field'].astype(np.float64) - ref) <= 2 * K * 2.0 ** -24 * mag).all()
    B, H, W = noise.shape
    pad = K // 2
    f64 = np.zeros((B, H, W))
    for b in range(B):
        g = run['taps'][b, :K].astype(np.float64)
        src = np.zeros((H + 2 * pad, W + 2 * pad))
        src[pad:pad + H, pad:pad + W] = noise[b]
        v = sum(g[k] * src[k:k + H] for k in range(K))
        f64[b] = sum(g[k] * v[:, k:k + W] for k in range(K))
    assert (np.abs(run['field'].astype(np.float64) - f64) <= 2 * K * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize('name', NAMES)
def test_model_passes_every_stage(name):
    run = _model(name)
    C.check_all(run, name, name, mask_in_place=run['mask'])
    if run['K'] == 1:
        assert np.array_equal(run['field'], C.noise_of(name))
    # the oracle's own field keeps to the band share of stage 7
    mask, field, thr, mean, std = C.oracle(name)
    assert C.band_share(field, thr, std) < 1e-3


def test_model_beyond_kcap():
    name, shape, sig = C.BEYOND
    run = C.device_model(C.noise_of(name), np.asarray(sig, F32), np.asarray([0.5], F32))
    C.check_taps(run, np.asarray(sig, F32), name)
    C.check_beyond_kcap(run, 0, name)


@pytest.mark.parametrize('at', C.IMPULSE_AT, ids=[f'{y}-{x}' for y, x in C.IMPULSE_AT])
def test_model_impulse(at):
    run = _model('impulse', at)
    C.check_impulse(run, at, f'impulse {at}')
    C.check_all(run, 'impulse', f'impulse {at}', variant=at)
    assert run['field'].sum() > 0
    bad = _model('impulse', at, mutate='centred')
    with pytest.raises(AssertionError):
        C.check_impulse(dict(bad, taps=run['taps']), at, 'mutant')


def test_designed_statistics():
    """integers -3 .. 3 through a K = 1 window: the field is the noise, both sums are integers far below 2^53 (exact
    in any order), no value lies within 1e-3 of a threshold at p = 1/2 or 0.3 (an ulp is 1e-7), p = 0 and 1 give
    infinite thresholds; the 'tie' variant sums to 0 exactly and holds zeros, which sit ON the threshold at p = 1/2"""
    n = C.noise_of('designed-stats')
    B = n.shape[0]
    assert np.array_equal(n, np.rint(n)) and np.abs(n).max() == 3
    run = _model('designed-stats', p=np.asarray([0.5, 0.3], F32))
    assert np.array_equal(run['field'], n)
    s1, s2 = n.reshape(B, -1).astype(np.int64).sum(1), (n.reshape(B, -1).astype(np.int64) ** 2).sum(1)
    assert np.array_equal(run['stats'], np.stack([s1, s2], 1).astype(np.float64))
    ref, M, meanf = C.thr_reference(run['stats'], np.asarray([0.5, 0.3], F32), float(n[0].size))
    for p in ((0.5, 0.5), (0.3, 0.3)):
        ref, _, _ = C.thr_reference(run['stats'], np.asarray(p, F32), float(n[0].size))
        assert np.abs(n - ref.reshape(B, 1, 1)).min() > 1e-3
    C.check_all(run, 'designed-stats', 'designed', p=np.asarray([0.5, 0.3], F32))
    ends = _model('designed-stats', p=np.asarray([0.0, 1.0], F32))
    assert ends['thr'][0] == -np.inf and ends['thr'][1] == np.inf
    assert (ends['mask'][0] == 1).all() and (ends['mask'][1] == 0).all()
    C.check_stats(ends, np.asarray([0.0, 1.0], F32), 'p = 0, 1')
    C.check_mask(ends, 'p = 0, 1')
    t = C.noise_of('designed-stats', 'tie')
    assert (t.reshape(B, -1).sum(1) == 0).all() and (t == 0).reshape(B, -1).sum(1).min() > 5 and np.abs(t).max() == 3


# ---------------------------------------------------------------------------------------------------------------------
# every check rejects its mutation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['half-1.5', 'k129', 'multi-sigma'])
def test_rejects_a_centred_tap_grid(name):
    run = _model(name, mutate='centred')
    with pytest.raises(AssertionError):
        C.check_taps(run, C.sigmas_of(C.CASE_BY_NAME[name]), 'mutant')
    good = _model(name)
    with pytest.raises(AssertionError):
        C.check_blur(dict(good, tmp=run['tmp']), C.noise_of(name), 'mutant')


def test_rejects_round_half_up():
    for name, differs in (('half-0.5', False), ('half-1.5', True), ('half-2.5', False)):
        run = _model(name, mutate='half-up')
        sig = C.sigmas_of(C.CASE_BY_NAME[name])
        if differs:
            with pytest.raises(AssertionError, match='K'):
                C.check_taps(run, sig, 'mutant')
        else:
            C.check_taps(run, sig, 'agrees')
    # half-down is caught by the other two
    for name in ('half-0.5', 'half-2.5'):
        sig = C.sigmas_of(C.CASE_BY_NAME[name])
        run = dict(_model(name), K=C.window_half_down(sig))
        with pytest.raises(AssertionError, match='K'):
            C.check_taps(run, sig, 'mutant')


def test_rejects_the_taps_of_sample_zero_for_every_sample():
    run = _model('multi-sigma', mutate='taps0')
    noise = C.noise_of('multi-sigma')
    with pytest.raises(AssertionError, match='vertical'):
        C.check_blur(run, noise, 'mutant')
    good = _model('multi-sigma')
    with pytest.raises(AssertionError, match='horizontal'):
        C.check_blur(dict(good, field=run['field']), noise, 'mutant')


@pytest.mark.parametrize('name', ['half-2.5', 'k129', 'ragged-63x255'])
def test_rejects_descending_tap_order(name):
    run = _model(name, mutate='descending')
    good = _model(name)
    assert not np.array_equal(run['tmp'], good['tmp'])
    with pytest.raises(AssertionError, match='vertical'):
        C.check_blur(run, C.noise_of(name), 'mutant')
    hz = C.blur_restate(good['tmp'], good['taps'], good['K'], 2, descending=True)
    with pytest.raises(AssertionError, match='horizontal'):
        C.check_blur(dict(good, field=hz), C.noise_of(name), 'mutant')


@pytest.mark.parametrize('name', ['k1', 'half-0.5', 'ragged-7x261'])
def test_rejects_a_biased_variance(name):
    run = _model(name, mutate='biased')
    with pytest.raises(AssertionError, match='thr'):
        C.check_stats(run, C.p_of(C.CASE_BY_NAME[name]), 'mutant')
    good = _model(name)
    bad = dict(good, stats=good['stats'] * np.array([1.0, 1 + 1e-12]))
    with pytest.raises(AssertionError, match='stats'):
        C.check_stats(bad, C.p_of(C.CASE_BY_NAME[name]), 'mutant')


def test_rejects_greater_or_equal():
    p = np.asarray([0.5, 0.5], F32)
    good, bad = _model('designed-stats', 'tie', p), _model('designed-stats', 'tie', p, mutate='ge')
    assert (good['thr'] == 0).all() and (good['field'] == 0).any()
    C.check_mask(good, 'tie')
    with pytest.raises(AssertionError, match='mask'):
        C.check_mask(bad, 'mutant')
    # a mask that is right everywhere but at one pixel inside the old tie band
    one = dict(good, mask=good['mask'].copy())
    one['mask'][1, 4, 7] = 1 - one['mask'][1, 4, 7]
    with pytest.raises(AssertionError, match='mask'):
        C.check_mask(one, 'mutant')
