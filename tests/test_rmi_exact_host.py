"""Keeps tests/exact_rmi.py honest without a GPU: every geometry has the property its row of GEOS is there for, the
restatements agree with the oracle and with torch on random data, the designed-operand facts hold in fp32 / fp64, a host
model of the device passes every stage check, and every stage check rejects the mutation it exists for when the mutant's
output is fed to it as the device result."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_rmi as R

F32 = np.float32
IDS = [R.geo_id(c) for c in R.GEOS]


def _geo(*case):
    assert case in R.GEOS
    return R.Geo(case)


def test_every_geometry_has_its_edge():
    g = _geo(33, 2, 12, 12, 2, 3, 2)
    assert g.NC == 66 and (g.NC + R.SOLVE_LANES - 1) // R.SOLVE_LANES == 2 and g.NC % R.SOLVE_LANES == 2
    g = _geo(1, 2, 66, 66, 2, 3, 0)
    assert (g.P, g.chunks, g.per) == (4096, 1, 4096)
    g = _geo(1, 2, 66, 67, 2, 3, 0)
    assert (g.P, g.chunks, g.per) == (4160, 2, 2080)
    g = _geo(1, 2, 726, 726, 2, 3, 0)
    assert g.P == 524176 and (g.P + R.POS_PER_BLOCK - 1) // R.POS_PER_BLOCK > 64 and g.chunks == 64
    assert g.cells == 1054152 and g.sweeps(g.cells) == 2 and g.sweeps(g.NC * g.H * g.W) == 2
    g = _geo(2, 2, 3, 40, 2, 3, 0)
    assert (g.Hv, g.Wv) == (1, 38)
    g = _geo(2, 2, 40, 3, 2, 3, 0)
    assert (g.Hv, g.Wv) == (38, 1)
    g = _geo(2, 2, 3, 3, 2, 3, 0)
    assert g.P == 1
    g = _geo(2, 3, 29, 31, 3, 2, 3)
    # odd window, pad 1: the windows tile rows -1 .. 28 and columns -1 .. 31, so every pixel of the 29 x 31 image is
    # covered and only the bottom padding row is not; the uncovered image rows / columns are live in the next two
    assert (g.k, g.pad, g.D) == (3, 1, 4) and (g.Hp - 1) * g.s - g.pad + g.k == g.H < g.H + g.pad
    assert (g.H - 1 + g.pad) // g.s < g.Hp and (g.W - 1 + g.pad) // g.s < g.Wp
    g = _geo(2, 2, 30, 27, 2, 2, 5)
    assert (g.k, g.pad) == (5, 2) and (g.H - 1 + g.pad) // g.s >= g.Hp      # the last rows uncovered
    g = _geo(2, 2, 21, 19, 2, 1, 4)
    assert g.D == 1 and g.k % 2 == 0 and (g.W - 1 + g.pad) // g.s >= g.Wp   # the last columns uncovered
    for ncls, rows in ((2, 6), (6, 2)):
        g = _geo(3, 4, 20, 20, ncls, 3, 2)
        assert g.rows == rows and g.C != ncls
    # the divisor differs from the number of pixels inside the image wherever a window hangs over the border
    for case in R.GEOS:
        g = R.Geo(case)
        assert (g.divisor() >= g.valid_count()).all() and (g.valid_count() >= 1).all()
        assert bool((g.divisor() != g.valid_count()).any()) == (g.pad > 0)
        lay, total = R.ws_layout(g)
        assert all(o % 256 == 0 for o, _, _ in lay.values()) and total % 256 == 0


def test_designed_sigmoid_is_exact_in_fp32():
    """for any faithful expf (the correctly rounded value or either neighbour): sigmoid(-30) clamps to 1e-6f,
    sigmoid(0) = 1/2, sigmoid(30) = 1"""
    for x, want in ((-30.0, R.CLIP_MIN), (0.0, F32(0.5)), (30.0, F32(1.0))):
        e = F32(np.exp(np.float64(-x)))
        for ee in (np.nextafter(e, F32(0)), e, np.nextafter(e, F32(np.inf))):
            if x == 0:
                ee = F32(1)
            y = F32(1) / (F32(1) + ee)
            got = min(max(y, R.CLIP_MIN), F32(1))
            assert got.view(np.uint32) == want.view(np.uint32), (x, ee, got)
    x = np.array([-30.0, 0.0, 30.0], F32)
    assert np.array_equal(R.probs32(x), R.designed_probs(x))
    assert np.array_equal(R.probs64(x).astype(F32), R.designed_probs(x))


@pytest.mark.parametrize('case', [c for c in R.GEOS if c != R.BIG], ids=[R.geo_id(c) for c in R.GEOS if c != R.BIG])
def test_pool_restatement_against_torch(case):
    """pool_restate is F.avg_pool2d: the bits on a 0/1 target, to 4 ulp on fp32 probabilities (the order of torch's
    CPU sum is its own), to 1e-15 in fp64"""
    g = R.Geo(case)
    x, t, _ = R.operands(case, 'random')
    if g.k == 1:
        assert np.array_equal(R.pool_restate(t, g), np.asarray(t).reshape(g.NC, g.H, g.W))
        return
    tt, pr = torch.from_numpy(np.array(t)), torch.from_numpy(R.probs32(x))
    assert np.array_equal(R.pool_restate(t, g), F.avg_pool2d(tt, g.k, g.s, g.pad).numpy().reshape(g.NC, g.Hp, g.Wp))
    ref = F.avg_pool2d(pr, g.k, g.s, g.pad).numpy().reshape(g.NC, g.Hp, g.Wp)
    np.testing.assert_allclose(R.pool_restate(pr.numpy(), g), ref, rtol=4 * 2.0 ** -23, atol=0)
    ref64 = F.avg_pool2d(pr.double(), g.k, g.s, g.pad).numpy().reshape(g.NC, g.Hp, g.Wp)
    np.testing.assert_allclose(R.pool_restate(pr.numpy(), g, np.float64), ref64, rtol=1e-15, atol=0)


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', R.GEOS, ids=IDS)
def test_model_passes_every_stage(case, kind):
    run = R.device_model(case, kind)
    R.check_all(run, case, kind, f'{R.geo_id(case)} {kind}', cov_series=[0] if case == R.BIG else None)


@pytest.mark.parametrize('kind', ['absent', 'absent2', 'saturated'])
def test_model_passes_the_special_cases(kind):
    """absent class: M = 0 for the series of channel 1, whose rmi is the closed form whatever the logits; saturated
    channel: S = 0 before the regulariser"""
    g = R.Geo(R.SPECIAL_GEO)
    run = R.device_model(R.SPECIAL_GEO, kind)
    R.check_all(run, R.SPECIAL_GEO, kind, kind)
    Lc, S, M = R.sum_chunks(run['part'], g)
    sel = np.arange(g.NC) % g.C == (0 if kind == 'saturated' else 1)
    assert (M[sel] == 0).all() and (run['coef'][sel] == 0).all() and (run['gx'].reshape(g.NC, -1)[sel] == 0).all()
    if kind == 'saturated':
        assert (S[sel] == 0).all() and (run['pp'][sel] == 1).all()
    else:
        assert (Lc[sel] == 0).all() and np.abs(run['rmi'][sel] - R.closed_form_p1(g)).max() <= R.closed_form_bound(g)


def test_designed_label_means_are_in_the_exact_class():
    """on designed operands every label mean is held to bit equality at every geometry (0/1 sums), and so is every
    probability mean wherever P < 1024 (values are multiples of 2^-43 at the least, sums below 2^10)"""
    for case in R.GEOS:
        g = R.Geo(case)
        n = R.check_means(R.device_model(case, 'designed'), g, R.geo_id(case))
        assert n >= g.NC * g.D
        if g.P < 1024 and g.k == 1:
            assert n == 2 * g.NC * g.D


def test_p_one_closed_form():
    g = R.Geo(R.P_ONE)
    run = R.device_model(R.P_ONE, 'random')
    cf = R.closed_form_p1(g)
    assert np.abs(run['rmi'] - cf).max() <= R.closed_form_bound(g)
    assert (run['coef'] == 0).all() and (run['gp'] == 0).all() and (run['gx'] == 0).all()
    assert float(run['loss']) == pytest.approx(2 * cf / g.D, rel=1e-6)
    ref_l, ref_g = R.oracle(R.P_ONE, 'random')
    assert (ref_g == 0).all()


def test_solve_against_mpmath_and_the_oracle():
    """the long double restatement against a 50-digit solve of the same covariances (its own error: far under the
    fp64 routes'), and the per-series rmi of both fp64 routes against the oracle's value on the same inputs"""
    mp = pytest.importorskip('mpmath')
    case = (3, 4, 20, 20, 2, 3, 2)
    g = R.Geo(case)
    run = R.device_model(case, 'random')
    Lc, S, M = R.sum_chunks(run['part'], g)
    ref_r, ref_q, ref_k, _ = R.solve_chol(Lc, S, M, R.LD)
    c_r, c_q, c_k, _ = R.solve_chol(Lc, S, M, np.float64)
    i_r, i_q, i_k = R.solve_inverse(Lc, S, M)
    mp.mp.dps = 50
    D = g.D
    worst = [0.0, 0.0, 0.0]
    for nc in (0, 5, 11):
        mS = mp.matrix(S[nc].tolist()) + mp.mpf(R.POS_ALPHA) * mp.eye(D)
        mM, mL = mp.matrix(M[nc].tolist()), mp.matrix(Lc[nc].tolist())
        Si = mp.inverse(mS)
        Aa = mL - mM * Si * mM.T + mp.mpf(R.POS_ALPHA) * mp.eye(D)
        La = mp.cholesky(Aa)
        rmi = sum(mp.log(La[i, i] + mp.mpf(R.DIAG_EPS)) for i in range(D))
        Li = mp.inverse(La)
        Gm = Li.T * mp.diag([La[i, i] / (La[i, i] + mp.mpf(R.DIAG_EPS)) for i in range(D)]) * Li
        Km = Si * mM.T * Gm
        Qm = Km * mM * Si
        kq = max(abs(Qm[i, j]) for i in range(D) for j in range(D))
        kk = max(abs(Km[i, j]) for i in range(D) for j in range(D))
        worst[0] = max(worst[0], float(abs(mp.mpf(float(ref_r[nc])) - rmi)))   # (the fp64 image of the long double)
        worst[1] = max(worst[1], float(max(abs(mp.mpf(float(ref_q[nc, i, j])) - Qm[i, j])
                                           for i in range(D) for j in range(D)) / kq))
        worst[2] = max(worst[2], float(max(abs(mp.mpf(float(ref_k[nc, i, j])) - Km[i, j])
                                           for i in range(D) for j in range(D)) / kk))
        for route in (c_r, i_r):
            assert abs(mp.mpf(float(route[nc])) - rmi) < 1e-12
    print('long double restatement (read back in fp64) against mpmath: rmi abs, Q rel, K rel', worst)
    # read back through fp64, the long double result is the correctly rounded fp64 of the 50-digit one, give or take
    assert worst[0] <= 2.0 ** -52 * 40 and worst[1] <= 2.0 ** -51 and worst[2] <= 2.0 ** -51
    # and the routes reproduce the oracle's loss on the inputs themselves
    x, t, gout = R.operands(case, 'random')
    ref_l, _ = R.oracle(case, 'random')
    for route in (c_r, i_r, ref_r.astype(np.float64)):
        assert float(R.loss_restate(route, g)) == pytest.approx(float(ref_l), rel=2e-6)


# ---------------------------------------------------------------------------------------------------------------------
# every check rejects its mutation
# ---------------------------------------------------------------------------------------------------------------------
AVG = (33, 2, 12, 12, 2, 3, 2)
TWO_CHUNKS = (1, 2, 66, 67, 2, 3, 0)


@pytest.mark.parametrize('kind', R.KINDS)
def test_rejects_the_divisor_without_padding(kind):
    g = R.Geo(AVG)
    x, t, _ = R.operands(AVG, kind)
    run = R.device_model(AVG, kind, mutate='divisor')
    with pytest.raises(AssertionError):
        R.check_pool(run, x, t, g, kind == 'designed', 'mutant')
    good = R.device_model(AVG, kind)
    bad = dict(good, lp=run['lp'])
    with pytest.raises(AssertionError):
        R.check_pool(bad, x, t, g, kind == 'designed', 'mutant lp')
    bad = dict(good, pp=run['pp'])
    with pytest.raises(AssertionError):
        R.check_pool(bad, x, t, g, kind == 'designed', 'mutant pp')
    # and the input gradient's divisor: gx from the GOOD pooled gradient, divided by the number of pixels inside the image
    mut = R.gx_model(good['gp'], x, g, g.valid_count())
    assert np.array_equal(R.gx_model(good['gp'], x, g, g.divisor()), good['gx'])
    x3 = np.asarray(x).reshape(g.NC, g.H, g.W)
    differs = mut.reshape(x3.shape) != good['gx'].reshape(x3.shape)
    assert (differs & (x3 == 0)).any() if kind == 'designed' else differs.any()   # border pixels at logit 0 among them
    with pytest.raises(AssertionError, match='gx'):
        R.check_gx(dict(good, gx=mut), x, g, kind == 'designed', 'mutant gx')


@pytest.mark.parametrize('case', [AVG, (2, 3, 29, 31, 3, 2, 3)], ids=['r3', 'r2'])
def test_rejects_a_crop_shifted_by_one(case):
    g = R.Geo(case)
    x, t, gout = R.operands(case, 'random')
    run = R.device_model(case, 'random', mutate='crop-shift')
    good = R.device_model(case, 'random')
    with pytest.raises(AssertionError):
        R.check_means(run, g, 'mutant')
    with pytest.raises(AssertionError):
        R.check_cov(dict(good, part=run['part']), g, 'mutant')
    with pytest.raises(AssertionError):
        R.check_gp(dict(good, gp=run['gp']), g, gout, 'mutant')


def test_rejects_a_chunk_that_takes_its_neighbours_position():
    g = R.Geo(TWO_CHUNKS)
    for kind in R.KINDS:
        run = R.device_model(TWO_CHUNKS, kind, mutate='chunk-leak')
        with pytest.raises(AssertionError):
            R.check_cov(run, g, 'mutant')
        R.check_cov(R.device_model(TWO_CHUNKS, kind), g, 'model')


@pytest.mark.parametrize('mutate', ['K-transposed', 'Q-from-M'])
def test_rejects_wrong_coefficients(mutate):
    g = R.Geo(AVG)
    run = R.device_model(AVG, 'random', mutate=mutate)
    cov = R.sum_chunks(run['part'], g)
    with pytest.raises(AssertionError, match='K' if mutate == 'K-transposed' else 'Q'):
        R.check_solve(run, g, cov, 'mutant')
    # one wrong series out of 66 in the per-series rmi: what the fp32 scalar hides, the stage check sees
    good = R.device_model(AVG, 'random')
    bad = dict(good, rmi=good['rmi'].copy())
    bad['rmi'][37] *= 1 + 1e-9
    assert float(R.loss_restate(bad['rmi'], g)) == float(good['loss'])
    with pytest.raises(AssertionError, match='rmi'):
        R.check_solve(bad, g, cov, 'mutant')


def test_rejects_a_wrong_loss_order_and_gradient_scale():
    """three faults of rmi_loss_kernel: the class sums divided by num_classes in place of the number of rows (6 and 2
    here); the class means added in fp64 and rounded once; the division by D done in fp64 before the cast.  Each is first shown to change the fp32
    scalar (the last two on the geometries where they do: at least one each), then to be rejected."""
    g = R.Geo((3, 4, 20, 20, 6, 3, 2))
    run = R.device_model(g.case, 'random')
    swapped = R.loss_restate(run['rmi'], R.Geo((3, 4, 20, 20, 2, 3, 2)))
    assert float(swapped) != float(run['loss'])
    with pytest.raises(AssertionError, match='loss'):
        R.check_loss(dict(run, loss=swapped), g, 'mutant')
    hit = {'once': 0, 'late': 0}
    for case in R.GEOS:
        if case == R.BIG:
            continue
        gg = R.Geo(case)
        for kind in R.KINDS:
            rr = R.device_model(case, kind)
            means = rr['rmi'].reshape(gg.rows, gg.ncls).sum(0) / gg.rows
            for name, bad in (('once', F32((means / gg.D).sum())),
                              ('late', sum((F32(m / gg.D) for m in means), F32(0)))):
                if float(bad) != float(rr['loss']):
                    hit[name] += 1
                    with pytest.raises(AssertionError, match='loss'):
                        R.check_loss(dict(rr, loss=F32(bad)), gg, 'mutant')
    print('geometries on which the one-rounding / late-division forms change the scalar:', hit)
    assert hit['once'] >= 1 and hit['late'] >= 1
    _, _, gout = R.operands(g.case, 'random')
    bad = dict(run, gp=(run['gp'] * F32(1 + 2.0 ** -18)).astype(F32))
    assert not np.array_equal(bad['gp'], run['gp'])
    with pytest.raises(AssertionError):
        R.check_gp(bad, g, gout, 'mutant')


def test_decode_rejects_a_changed_layout():
    g = R.Geo(AVG)
    _, total = R.ws_layout(g)
    ws = np.zeros(total, np.uint8)
    R.decode(ws, g, total)
    with pytest.raises(AssertionError, match='layout'):
        R.decode(ws, g, total + 256)
    assert math.isfinite(R.closed_form_p1(g))
