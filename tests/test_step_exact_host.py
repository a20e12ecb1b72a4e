"""Keeps tests/exact_step.py honest without a GPU: fma32 against exact rationals, every restatement against an
independent computation (the reference's golden, torch's fp64 optimizer, a sequence written out by hand), the operand
sets non-degenerate and inside the ranges the exact comparisons need, and every comparison function of
test_step_exact.py rejecting the fault it exists for when it is fed a mutant's output as the device result."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact as E
import exact_step as S
from conftest import golden

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# fma32
# ---------------------------------------------------------------------------------------------------------------------
def _round_f32(fr):
    """the fp32 value nearest to the rational fr, ties to even, by exact comparison of the neighbours"""
    c = np.float32(float(fr))   # Fraction -> float is correctly rounded; its fp32 rounding is within one step
    cands = {float(c), float(np.nextafter(c, F32(np.inf))), float(np.nextafter(c, F32(-np.inf)))}
    cands = [v for v in cands if np.isfinite(v)]
    best = min(abs(Fraction(v) - fr) for v in cands)
    tied = [v for v in cands if abs(Fraction(v) - fr) == best]
    if len(tied) > 1:
        tied = [v for v in tied if (int(np.float32(v).view(np.uint32)) & 1) == 0]
    return np.float32(tied[0])


def _tie_triples():
    """(1 + k 2^-12)^2 = 1 + k 2^-11 + k^2 2^-24 with k odd is an exact fp32 midpoint; c = +-2^-60 decides it, and
    is lost in the fp64 sum"""
    out = []
    for k in range(1, 200, 2):
        a = 1 + k * 2.0 ** -12
        for sa in (1.0, -1.0):
            for c in (2.0 ** -60, -2.0 ** -60):
                out.append((sa * a, a, c))
    return np.array(out, dtype=np.float64).astype(np.float32)


def test_fma32_against_fractions():
    rng = np.random.default_rng(11)
    n = 12000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    c[: n // 4] = -(a[: n // 4] * b[: n // 4])          # cancellation: the sum is the product's rounding error
    c[n // 4: n // 2] *= np.float32(2.0 ** -30)         # an addend far below the product's last bit
    got = S.fma32(a, b, c)
    bad = sum(int(_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))).view(np.uint32)
                  != g.view(np.uint32)) for x, y, z, g in zip(a, b, c, got))
    assert bad == 0, f'{bad} of {n} random triples'

    t = _tie_triples()
    got, naive = S.fma32(t[:, 0], t[:, 1], t[:, 2]), S.fma32_naive(t[:, 0], t[:, 1], t[:, 2])
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in t])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the constructed ties break both ways, and the double rounding is wrong on a full half of them (the side its
    # tie rule does not happen to pick) -- on every one whose true rounding is the odd neighbour
    mid = np.abs(t[:, 0].astype(np.float64) * t[:, 1].astype(np.float64))
    assert (np.abs(want) > mid).sum() == (np.abs(want) < mid).sum() == len(t) // 2
    odd = (want.view(np.uint32) & 1) == 1
    assert odd.sum() == len(t) // 2 and (naive[odd] != want[odd]).all() and (naive[~odd] == want[~odd]).all()


def test_bf16_rne_is_torchs_cast():
    x = S.values((4099,), 'f32').numpy()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = S.bf16_rne(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]) and ((got[nan] & 0x7fff) > 0x7f80).all()
    assert (S.bf16_trunc(x)[~nan] != want[~nan]).mean() > 0.3


# ---------------------------------------------------------------------------------------------------------------------
# EMA
# ---------------------------------------------------------------------------------------------------------------------
def test_ema_ref_reproduces_the_golden():
    g = golden('ema.npz')
    keys = [k[2:] for k in g.files if k.startswith('t.') and 'running' not in k and 'num_batches' not in k]
    e = np.concatenate([g['t.' + k].reshape(-1) for k in keys])
    p = np.concatenate([g['s.' + k].reshape(-1) for k in keys])
    ref = np.concatenate([g['after.' + k].reshape(-1) for k in keys])
    assert np.array_equal(S.ema_ref(e, p, float(g['alpha'])), ref)


@pytest.mark.parametrize('alpha', S.EMA_ALPHAS)
def test_ema_mutation_is_rejected(alpha):
    assert F32(1.0) - F32(alpha) != F32(1.0 - alpha)
    e, p = S.ema_operands(1023)
    S.ema_check(S.ema_ref(e, p, alpha), e, p, alpha, 'ema')
    with pytest.raises(AssertionError):
        S.ema_check(S.ema_ref(e, p, alpha, mutate='beta32'), e, p, alpha, 'ema beta32')


# ---------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------
def _torch_sgd64(p, grads, lr, mom, wd, max_norm):
    """clip_grad_norm_ + torch.optim.SGD in fp64; returns per step (p, buf, clipped g)"""
    q = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd)
    out = []
    for g in grads:
        q.grad = torch.from_numpy(g.astype(np.float64))
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([q], max_norm)
        opt.step()
        buf = opt.state[q].get('momentum_buffer')
        out.append((q.detach().numpy().copy(), None if buf is None else buf.numpy().copy(), q.grad.numpy().copy()))
    return out


@pytest.mark.parametrize('contract', (True, False), ids=['fma', 'two-roundings'])
@pytest.mark.parametrize('mom,wd', [(0.9, 5e-4), (0.0, 5e-4), (0.9, 0.0)])
def test_sgd_ref_follows_torch_fp64(mom, wd, contract):
    """sgd_ref, with coef = float32(clip_coef_ref(fp64 norm)), against clip_grad_norm_ + torch.optim.SGD run in fp64 on
    the same fp32 inputs and the same (float32-valued) hyperparameters, 3 steps.  Per element and per step, with
    u = 2^-24 and E_x the bound carried for x (E_p = E_buf = 0 at the start), first order in u with the magnitudes
    taken from the fp64 run plus their own bound:
        E_gi  = 2 u |gi|                                   (the coefficient's rounding, the product)
        E_d   = wd E_p + E_gi + u |d|                      (one fma)
        E_b   = mom (E_buf + u |buf|) + E_d + u |b|        (the sum, and the product's rounding where the momentum
                                                           update is not contracted; E_b = E_d on the first step)
        E_p'  = E_p + lr E_b + u |p'|                      (one fma)
    """
    rng = np.random.default_rng(5)
    n = 1027
    p = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 3).astype(np.float32) for _ in range(3)]
    lr, mom, wd = (float(F32(v)) for v in (0.05, mom, wd))
    max_norm = float(F32(0.25 * np.sqrt(np.sum(grads[0].astype(np.float64) ** 2))))
    ref = _torch_sgd64(p, grads, lr, mom, wd, max_norm)
    u = S.U24
    buf = np.zeros(n, np.float32)
    Ep = Ebuf = np.zeros(n)
    prev_p, prev_buf = p.astype(np.float64), None
    for t, g in enumerate(grads):
        coef = F32(S.clip_coef_ref(np.sum(g.astype(np.float64) ** 2), max_norm, 1.0))
        p, gi, nbuf, _ = S.sgd_ref(p, g, buf, coef, lr, mom, wd, t == 0, False, contract=contract)
        rp, rbuf, rg = ref[t]
        mag = lambda r, e: np.abs(r) + e  # noqa: E731
        Egi = 2 * u * np.abs(rg) * (1 + 4 * u)
        rd = rg + wd * prev_p
        Ed = wd * Ep + Egi + u * mag(rd, wd * Ep + Egi)
        if mom != 0:
            rb = rbuf
            Eb = Ed if t == 0 else mom * (Ebuf + u * mag(prev_buf, Ebuf)) + Ed + u * mag(rb, mom * Ebuf + Ed)
            assert (np.abs(nbuf - rb) <= Eb).all(), ('buf', t)
            buf, Ebuf = nbuf, Eb
        else:
            Eb = Ed
        Ep = Ep + lr * Eb + u * mag(rp, Ep + lr * Eb)
        assert (np.abs(gi - rg) <= Egi).all(), ('g', t)
        assert (np.abs(p.astype(np.float64) - rp) <= Ep).all(), ('p', t)
        # the bound is tight enough to mean something: a few ulp of the parameters
        assert Ep.max() <= 16 * u * np.abs(rp).max()
        prev_p, prev_buf = rp, rbuf


def test_sgd_ref_is_exact_on_dyadic_operands():
    """Small integers times powers of two with power-of-two lr, wd, momentum and coefficient: every intermediate of 3
    steps is representable (check_exact_range), so sgd_ref EQUALS the fp64 optimizer."""
    g_ = E._gen('sgd-dyadic')
    n = 515
    p = E.ints((n,), -8, 8, 1.0, g_).numpy().astype(np.float32)
    grads = [(E.ints((n,), -8, 8, 1.0, g_) * 2.0).numpy().astype(np.float32) for _ in range(3)]
    lr, mom, wd, coef = 2.0 ** -2, 0.5, 2.0 ** -3, 0.5
    ref = _torch_sgd64(p, [g * coef for g in grads], lr, mom, wd, 0.0)
    buf = np.zeros(n, np.float32)
    for t, g in enumerate(grads):
        p, gi, buf, sh = S.sgd_ref(p, g, buf, coef, lr, mom, wd, t == 0, True)
        rp, rbuf, rg = ref[t]
        E.check_exact_range({'p': torch.from_numpy(rp), 'buf': torch.from_numpy(rbuf), 'g': torch.from_numpy(rg)},
                            'f32', 15)
        assert np.array_equal(p.astype(np.float64), rp) and np.array_equal(buf.astype(np.float64), rbuf)
        assert np.array_equal(gi.astype(np.float64), rg)
        assert np.array_equal(sh, S.bf16_rne(rp.astype(np.float32)))
    assert len(np.unique(p)) > 100


def _sgd_model_case(n, mom, wd, clip, amp, first, shadow, mutate=None):
    op = S.sgd_operands(n, amp)
    mx = S.sgd_max_norm(op, clip)
    got = S.sgd_device_model(op, mom, wd, mx, amp, first, shadow, mutate)
    S.sgd_check(got, op, mom, wd, mx, amp, first, f'sgd {mutate}')


@pytest.mark.parametrize('n', S.SGD_SIZES[:3] + (S.SGD_N,))
@pytest.mark.parametrize('clip', S.SGD_CLIP)
@pytest.mark.parametrize('amp', S.SGD_AMP)
def test_sgd_check_accepts_the_device_model(n, clip, amp):
    """a float32 evaluation of the kernel's own coefficient lines passes (a) with room, and (b) by construction"""
    for mom, wd, first in ((0.9, 5e-4, 0), (0.9, 5e-4, 1), (0.0, 0.0, 0)):
        _sgd_model_case(n, mom, wd, clip, amp, first, True)


@pytest.mark.parametrize('mutate,n,first', [
    ('wd-after-momentum', S.SGD_N, 0), ('first-ignored', S.SGD_N, 1), ('unscale-late', S.SGD_N, 0),
    ('no-eps', 1, 0),    # 1e-6 against a norm of 1: 16.8 x 2^-24 relative; invisible against a norm of ~96 at n = 1027
    ('shadow-trunc', S.SGD_N, 0), ('g-not-written', S.SGD_N, 0),
    ('two-roundings', S.SGD_N, 0)])   # not a fault of the list: the form the device does NOT compute (sgd_ref)
def test_sgd_mutations_are_rejected(mutate, n, first):
    """each on the operand set and flags of a case test_step_exact.py runs: momentum, weight decay, a clip below the
    norm, the loss scale and the shadow all on"""
    with pytest.raises(AssertionError):
        _sgd_model_case(n, 0.9, 5e-4, 'below', True, first, True, mutate)


@pytest.mark.parametrize('amp', S.SGD_AMP)
@pytest.mark.parametrize('wd', S.SGD_WD)
def test_contracted_momentum_against_two_roundings(amp, wd):
    """What the single fma of the device (sgd_ref) changes against the two roundings the source suggests, on the
    n = 1027 operands after one non-first step: the momentum buffer differs in 15 to 25 % of the elements, by no more
    than the product's dropped rounding and the two final ones (2^-24 |buf mom| + 2^-23 |b|); 2 to 5 % of the parameters
    change, by lr times that and their own rounding.  DESIGN.md 20 quotes these shares."""
    op = S.sgd_operands(S.SGD_N, amp)
    args = (op['p'], op['g'], op['buf'], 1.0 / op['S'], S.SGD_LR, 0.9, wd, 0, False)
    (p1, _, b1, _), (p2, _, b2, _) = S.sgd_ref(*args, contract=True), S.sgd_ref(*args, contract=False)
    db = np.abs(b1.astype(np.float64) - b2)
    mag_b = np.maximum(np.abs(b1), np.abs(b2)).astype(np.float64)
    assert (db <= S.U24 * np.abs(op['buf'].astype(np.float64) * 0.9) * 1.001 + 2 * S.U24 * mag_b).all()
    assert 0.15 <= (db != 0).mean() <= 0.25, (db != 0).mean()
    dp = np.abs(p1.astype(np.float64) - p2)
    assert (dp <= S.SGD_LR * db * 1.001 + 2 * S.U24 * np.maximum(np.abs(p1), np.abs(p2))).all()
    assert 0.02 <= (dp != 0).mean() <= 0.05, (dp != 0).mean()


def test_sgd_operands():
    for n in S.SGD_SIZES:
        for amp in S.SGD_AMP:
            op = S.sgd_operands(n, amp)
            assert op['g'][0] == op['S'] and (op['buf'] != 0).all()
            assert np.isfinite(F32(op['sq'])) and op['norm'] >= 1.0
            for k in ('p', 'g', 'buf'):
                assert (op[k] != 0).mean() >= 0.5 and (n < 8 or len(np.unique(op[k])) > n // 2)
    # the grid-sweep constants are those of the launches (ssseg_grid; ssseg_ema_update, ssseg_sgd_step)
    assert S.SGD_SIZES[-1] > S.SWEEP_SGD and S.SQ_SIZES[-1] > S.SWEEP_RED
    # the EMA's float4 loop runs n // 4 items on at most SWEEP_EMA // 4 threads: a second iteration needs more items
    assert S.EMA_SIZES[-1] // 4 > S.SWEEP_EMA // 4 and S.EMA_SIZES[-1] % 4 == 3


def test_flat_operands_are_nondegenerate():
    """the EMA, axpby / scale and sigmoid operands: at least half nonzero, (nearly) all values distinct, the two
    operands of a pair different"""
    sets = [S.ema_operands(n) for n in S.EMA_SIZES[:5]] + [(S.vec(n, 'x'), S.vec(n, 'y')) for n in S.AXPBY_N[:2]]
    sets += [S.sigmoid_operands(S.SIGMOID_N[0]), (S.vec(257, 'g'), S.vec(257, 'scale-by'))]
    for a, b in sets:
        assert not np.array_equal(a, b)
        for v in (a, b):
            assert (v != 0).mean() >= 0.5 and len(np.unique(v)) >= 0.9 * v.size


# ---------------------------------------------------------------------------------------------------------------------
# squared norm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', S.SQ_SIZES)
def test_sq_operands(n):
    a, b = S.sq_ints(n, 0), S.sq_ints(n, 1)
    assert np.array_equal(a, np.round(a)) and not np.array_equal(a, b)
    total = float(np.sum(a.astype(np.float64) ** 2) + np.sum(b.astype(np.float64) ** 2))
    assert 0 < total < 2 ** 24 and np.sum(a ** 2) > 0
    x = S.sq_normals(n)
    ref = float(np.sum(x.astype(np.float64) ** 2))
    S.sq_check_bounded(F32(ref), x, 'sq')
    with pytest.raises(AssertionError):   # a dropped last element is seen
        S.sq_check_bounded(F32(ref - float(x[-1]) ** 2), x, 'sq tail') if n > 1 else S.sq_check_bounded(0.0, x, 'sq')


# ---------------------------------------------------------------------------------------------------------------------
# loss scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('growth', S.AMP_GROWTHS)
def test_amp_ref_follows_the_scripted_sequence(growth):
    states = S.amp_script(growth)
    assert len(states) == len(S.AMP_SCRIPT) == len(S.AMP_EXPECT[growth])
    for i, (st, (sc, tr, fi)) in enumerate(zip(states, S.AMP_EXPECT[growth])):
        want = np.array([sc, tr, fi, F32(1.0) / F32(sc)], dtype=np.float32)
        assert np.array_equal(st, want), (i, st, want)
    # the 1 / S slot sees a division that rounds
    if growth == 1.5:
        assert any(float(st[3]) * float(st[0]) != 1.0 for st in states)


# ---------------------------------------------------------------------------------------------------------------------
# axpby
# ---------------------------------------------------------------------------------------------------------------------
def test_axpby_ref():
    x, y = S.vec(257, 'x'), S.vec(257, 'y')
    for a, b in S.AXPBY_AB:
        got = S.axpby_ref(x, a, y, b).astype(np.float64)
        ref = float(F32(a)) * x.astype(np.float64) + float(F32(b)) * y.astype(np.float64)
        m = np.abs(float(F32(a)) * x) + np.abs(float(F32(b)) * y)
        assert (np.abs(got - ref) <= 2 * S.U24 * m).all()
    assert np.array_equal(S.axpby_ref(x, 1.0, y, 1.0), x + y)      # a = b = 1: the plain fp32 sum
    assert np.array_equal(S.axpby_ref(x, 0.1), x * F32(0.1)) and np.array_equal(S.scale_ref(x, 1 / 3), x * F32(1 / 3))


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt_in', S.DTYPES)
def test_layout_operands(dt_in):
    n, h, w = S.LAYOUT_NHW
    for C, Cp in S.GENERIC_CCP + S.PIXEL_CCP:
        x = S.values((n, C, h, w), dt_in)
        assert S.specials_present(x, dt_in)
        S.nondegenerate(x, f'x C{C}')
        src = S.values((n, h, w, Cp), dt_in, 'nhwc', lanes=C)
        assert S.specials_present(src[..., :C], dt_in)     # in the lanes the reader reads
        S.nondegenerate(src.permute(0, 3, 1, 2), f'nhwc Cp{Cp}')
    C, ldc = S.HEAD_VIEW
    assert S.specials_present(S.values((n, h, w, ldc), dt_in, 'nhwc', lanes=C)[..., :C], dt_in)
    bn, bC, bh, bw, bld = S.BIG_NCHW
    assert S.specials_present(S.values((bn, bh, bw, bld), dt_in, 'nhwc', lanes=bC)[..., :bC], dt_in)
    for m in S.CAST_N[1:]:
        assert S.specials_present(S.values((m,), dt_in), dt_in)
    assert len(S.SPECIALS) == S.SPECIAL_VALUES.numel() <= n * h * w


def test_special_values_do_what_their_names_say():
    s = {k: torch.tensor(v, dtype=torch.float32) for k, v in S.SPECIALS.items()}
    bf = lambda k: float(s[k].to(torch.bfloat16))  # noqa: E731
    hf = lambda k: float(s[k].to(torch.float16))  # noqa: E731
    assert all(float(v) == S.SPECIALS[k] or k == 'nan' for k, v in s.items())     # each is an fp32 value
    assert bf('bf16 tie down') == 1.0 and bf('bf16 tie up') == 1 + 2.0 ** -6 and bf('FLT_MAX') == float('inf')
    assert hf('f16 tie down') == 1.0 and hf('f16 tie up') == 1 + 2.0 ** -9
    assert hf('f16 overflow') == float('inf') and hf('f16 below overflow') == 65504.0
    assert hf('f16 sub') == 3 * 2.0 ** -24 and hf('f16 sub tie0') == 0.0 and hf('f16 sub tie up') == 2.0 ** -23
    assert hf('f16 sub inexact') == 2 * 2.0 ** -24 and hf('f16 sub under') == 0.0
    assert str(hf('f16 sub under')) == '-0.0'
    assert bf('f32 sub') == 2.0 ** -130 and bf('f32 sub tie') == -(2.0 ** -133) and bf('f32 min sub') == 0.0


@pytest.mark.parametrize('kind', ('pad', 'stride'))
def test_layout_mutations_are_rejected(kind):
    n, h, w = S.LAYOUT_NHW
    for (C, Cp), (di, do) in (((3, 8), ('f32', 'bf16')), ((5, 12), ('f16', 'f32')), ((3, 4), ('bf16', 'bf16'))):
        x = S.values((n, C, h, w), di)
        ref = S.to_nhwc_ref(x, Cp, do)
        S.same_bits_nan(ref.clone(), ref, 'layout')
        with pytest.raises(AssertionError):
            S.same_bits_nan(S.to_nhwc_mutant(x, Cp, do, kind, float('nan')), ref, f'layout {kind}')
    # a -0.0 in a padded lane is not +0.0
    bad = ref.clone()
    bad[0, 0, 0, -1] = -0.0
    with pytest.raises(AssertionError):
        S.same_bits_nan(bad, ref, 'layout -0')


# ---------------------------------------------------------------------------------------------------------------------
# sigmoid, mix
# ---------------------------------------------------------------------------------------------------------------------
def test_sigmoid_checks():
    x, gy = S.sigmoid_operands(S.SIGMOID_N[0])
    assert (x != 0).mean() > 0.5 and list(x[:len(S.SIGMOID_SPECIALS)]) == list(S.SIGMOID_SPECIALS)
    assert list(np.flatnonzero(S.sigmoid_overflows(x))) == [S.SIGMOID_SPECIALS.index(-90.0)]
    t = torch.from_numpy(x)
    y = torch.sigmoid(t.double()).float().numpy()
    y[S.sigmoid_overflows(x)] = 0.0
    S.sigmoid_check_fwd(y, x, 'sigmoid')
    S.sigmoid_check_bwd((gy.astype(np.float64) * y * (1.0 - y.astype(np.float64))).astype(np.float32), y, gy, 'bwd')
    with pytest.raises(AssertionError):   # sigmoid(-x)
        S.sigmoid_check_fwd(torch.sigmoid(-t.double()).float().numpy(), x, 'sigmoid -x')
    with pytest.raises(AssertionError):   # gy * v, the (1 - v) dropped
        S.sigmoid_check_bwd(gy * y, y, gy, 'bwd v')


@pytest.mark.parametrize('mode', E.MODES)
def test_mix_checks(mode):
    shape = S.MIX_SHAPES[0]
    a, b, m = S.mix_operands(shape, mode, False)
    S.nondegenerate(a, 'a')
    S.nondegenerate(b, 'b')
    assert not torch.equal(m[0], m[1]) and 0.2 < float(m.mean()) < 0.8 and set(m.flatten().tolist()) == {0.0, 1.0}
    S.mix_check_binary(S.mix_binary_ref(a, b, m), a, b, m, 'mix')
    # the plain expression gives the selected operand exactly
    assert torch.equal((a.float() * m + b.float() * (1 - m)).to(a.dtype), S.mix_binary_ref(a, b, m))
    with pytest.raises(AssertionError):
        S.mix_check_binary(S.mix_wrong_mask(a, b, m), a, b, m, 'mix mask[b * C + c]')
    a, b, m = S.mix_operands(shape, mode, True)
    assert float(m.min()) > 0 and float(m.max()) < 1
    v = (a.float() * m + b.float() * (1 - m)).to(a.dtype)
    S.mix_check_soft(v, a, b, m, mode, 'mix soft')
    with pytest.raises(AssertionError):   # the mask of the other image
        S.mix_check_soft((a.float() * m.flip(0) + b.float() * (1 - m.flip(0))).to(a.dtype), a, b, m, mode, 'flip')
