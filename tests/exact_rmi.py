"""Operands, host restatements and stage-by-stage comparison functions for the RMI loss kernels (csrc/rmi.hip;
test_rmi_exact*.py).  Nothing here imports ssseg: the comparison functions take the device's result as a plain dict of
host arrays (`run`), so the host file can feed them a model's or a mutant's output instead.

Every stage of the pipeline leaves its result in the caller's workspace (ws_layout, rmi.hip:335-352: pp, lp, gp, mean,
part, coef, rmi, each segment aligned to 256 bytes), so each stage is checked against ITS OWN inputs as the device
produced them; an error cannot hide behind the conditioning of a later stage.

  stage                   tier      check
  1 pooled labels lp      bits      fp32 avg_pool2d of a 0/1 target (integer sum, one correctly rounded division)
    pooled probs pp       bits      designed logits {-30, 0, 30}: window added in row-major order, one division
                          bounded   random logits: 1/2 ulp + (k k + 4) 2^-24 ref (check_pool)
  2 means                 bits      where the fp64 sum is provably exact in any order (check_means), else
                          bounded   (P - 1) 2^-53 sum|v| / P
  3 covariance partials   bounded   (P + chunks) 2^-53 sum|term| against a long double sum; symmetry; chunk ranges
  4 solve (rmi, Q, K)     measured  16 x the larger error of two fp64 host routes against long double, no floor
  5 loss scalar           bits      the kernel's order in fp64 / fp32 (rmi.hip:256-266)
  6 pooled gradient gp    bounded   1/2 ulp + (D + 1) 2^-24 M (check_gp)
  7 input gradient gx     bits      0 at +-30 and in uncovered rows / columns, (gp / div) / 4 at logit 0
                          bounded   random logits: 1/2 ulp + 2^-24 M (check_gx)

Measured figures of stage 4 (the worst over the series of a geometry, printed by check_solve; one MI355X, every
geometry of GEOS on designed and random operands, and the two special cases): the fp64 Cholesky route is within 9.8e-15
absolute of the long double rmi and 1.8e-14 relative of the coefficients, the torch.inverse route within 1.2e-14 and
2.4e-14, the device within 8.1e-15 and 1.7e-14 -- at most 2.0 x the larger host route on any geometry (bound 16 x).
Worst per geometry (rmi absolute | Q relative, larger host route -> device): 33x2x12x12 1.2e-14 -> 8.1e-15 | 2.1e-14 ->
1.7e-14; 66x66 5.6e-15 -> 5.6e-15 | 1.3e-15 -> 1.3e-15; 66x67 4.1e-15 -> 4.1e-15 | 1.2e-15 -> 1.2e-15; 726x726 6.0e-15
-> 6.0e-15 | 1.6e-15 -> 1.6e-15; 3x40 1.6e-15 -> 1.6e-15 | 1.7e-15 -> 2.1e-15; 40x3 1.3e-15 -> 1.2e-15 | 2.6e-15 ->
2.2e-15; 3x3 7.7e-15 -> 7.7e-15 | 0 -> 0; 29x31 6.6e-16 -> 4.4e-16 | 1.3e-15 -> 1.3e-15; 30x27 1.5e-15 -> 2.8e-15 |
2.4e-15 -> 4.8e-15; 21x19 2.6e-16 -> 2.6e-16 | 9.9e-16 -> 9.9e-16; 3x4x20x20 (2 and 6 classes) 2.4e-15 -> 2.4e-15 |
1.9e-15 -> 2.1e-15.  The long double restatement itself is within one fp64 ulp of a 50-digit mpmath solve of the same
covariances (test_rmi_exact_host.py).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import exact_aux as A
from exact import _gen
from exact_step import same_bits

F32 = np.float32
LD = np.longdouble
U53 = 2.0 ** -53
POS_ALPHA = 5e-4          # rmi.hip:29
DIAG_EPS = 1e-8           # rmi.hip:226
CLIP_MIN = F32(1e-6)      # rmi.hip:66
RT, POS_PER_BLOCK = 256, 256 * 16   # rmi.hip:27-30
SWEEP = 4096 * 256        # cells one grid-stride sweep of ssseg_grid(n, 256) covers
SOLVE_LANES = 64          # rmi.hip:386
SOLVE_MARGIN = 16.0

# (N, C, H, W, num_classes, radius, pool window; 0 = no pooling)
GEOS = (
    (33, 2, 12, 12, 2, 3, 2),
    (1, 2, 66, 66, 2, 3, 0),
    (1, 2, 66, 67, 2, 3, 0),
    (1, 2, 726, 726, 2, 3, 0),
    (2, 2, 3, 40, 2, 3, 0),
    (2, 2, 40, 3, 2, 3, 0),
    (2, 2, 3, 3, 2, 3, 0),
    (2, 3, 29, 31, 3, 2, 3),
    (2, 2, 30, 27, 2, 2, 5),
    (2, 2, 21, 19, 2, 1, 4),
    (3, 4, 20, 20, 2, 3, 2),
    (3, 4, 20, 20, 6, 3, 2),
)
BIG = (1, 2, 726, 726, 2, 3, 0)
P_ONE = (2, 2, 3, 3, 2, 3, 0)
SPECIAL_GEO = (1, 2, 66, 67, 2, 3, 0)    # the absent-class and saturated-channel cases
KINDS = ('designed', 'random')
GOUT = {'designed': 0.5, 'random': 0.75, 'absent': 0.75, 'absent2': 0.75, 'saturated': 0.75}


def geo_id(case):
    n, c, h, w, ncls, r, k = case
    return f'{n}x{c}x{h}x{w}-cls{ncls}-r{r}-' + (f'avg{k}' if k else 'none')


def pool_args(k):
    """(kernel, stride, padding) as losses.RMILoss.pool_params hands them to the kernel"""
    return (k, k, k // 2) if k else (1, 1, 0)


class Geo:
    """make_geo (rmi.hip:355-379) restated"""

    def __init__(self, case):
        N, C, H, W, ncls, r, kk = case
        k, s, pad = pool_args(kk)
        assert (N * C) % ncls == 0 and 1 <= r <= 3 and k == s and 0 <= pad < k
        self.case = case
        self.N, self.C, self.NC, self.H, self.W = N, C, N * C, H, W
        self.k, self.s, self.pad = k, s, pad
        self.Hp, self.Wp = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        self.r, self.D = r, r * r
        self.Hv, self.Wv = self.Hp - r + 1, self.Wp - r + 1
        assert self.Hv >= 1 and self.Wv >= 1
        self.P = self.Hv * self.Wv
        self.chunks = min(64, (self.P + POS_PER_BLOCK - 1) // POS_PER_BLOCK)
        self.per = (self.P + self.chunks - 1) // self.chunks
        self.ncls, self.rows = ncls, self.NC // ncls
        self.cells = self.NC * self.Hp * self.Wp
        self.args = (N, C, H, W, ncls, r, k, s, pad)     # the nine int64 of the entry points

    def sweeps(self, n):
        return (n + SWEEP - 1) // SWEEP

    def divisor(self):
        """[Hp, Wp] fp32: the padded window area, clipped at H + pad / W + pad (rmi.hip:54-56)"""
        h0 = np.arange(self.Hp) * self.s - self.pad
        w0 = np.arange(self.Wp) * self.s - self.pad
        dh = np.minimum(h0 + self.k, self.H + self.pad) - h0
        dw = np.minimum(w0 + self.k, self.W + self.pad) - w0
        return (dh[:, None] * dw[None, :]).astype(F32)

    def valid_count(self):
        """the mutation: the number of window pixels inside the image"""
        h0 = np.arange(self.Hp) * self.s - self.pad
        w0 = np.arange(self.Wp) * self.s - self.pad
        dh = np.minimum(h0 + self.k, self.H) - np.maximum(h0, 0)
        dw = np.minimum(w0 + self.k, self.W) - np.maximum(w0, 0)
        return (dh[:, None] * dw[None, :]).astype(F32)


def _a256(b):
    return (b + 255) & ~255


def ws_layout(g):
    """ws_layout (rmi.hip:335-352): name -> (byte offset, dtype, shape), and the total"""
    segs = (('pp', F32, (g.NC, g.Hp, g.Wp)), ('lp', F32, (g.NC, g.Hp, g.Wp)), ('gp', F32, (g.NC, g.Hp, g.Wp)),
            ('mean', np.float64, (g.NC, 2 * g.D)), ('part', np.float64, (g.NC, g.D, g.chunks, 3 * g.D)),
            ('coef', np.float64, (g.NC, 2, g.D, g.D)), ('rmi', np.float64, (g.NC,)))
    out, o = {}, 0
    for name, dt, shape in segs:
        out[name] = (o, dt, shape)
        o += _a256(int(np.prod(shape)) * np.dtype(dt).itemsize)
    return out, o


def decode(ws_bytes, g, expect_total):
    """the workspace (uint8 host array) as named arrays; the restated total must be the library's"""
    lay, total = ws_layout(g)
    assert total == expect_total, f'workspace layout changed: restated {total} bytes, library says {expect_total}'
    assert ws_bytes.dtype == np.uint8 and ws_bytes.size >= total
    out = {}
    for name, (o, dt, shape) in lay.items():
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = ws_bytes[o:o + n].view(dt).reshape(shape).copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(case, kind):
    """(logits, target, gout) fp32 [N, C, H, W]; read-only.
    designed: logits from {-30, 0, 30} (2/5 zero, 2/5 agreeing with the target, 1/5 against it), an iid 0/1 target,
    gout = 1/2.  random: 2.5 randn + 1.5 (2 t - 1), clipped to [-12, 12] so that no sigmoid comes near the clamp at
    1e-6 (x = -13.8) or rounds to 1 (x > 16.6), where an fp32 and an fp64 sigmoid may take different branches;
    gout = 3/4.  absent / absent2: random with label channel 1 all zero (absent2 redraws that channel's logits);
    saturated: random with logit channel 0 all +30."""
    N, C, H, W = case[:4]
    base = 'random' if kind in ('absent', 'absent2', 'saturated') else kind
    g = _gen('rmi', case, base)
    t = (torch.rand(N, C, H, W, generator=g) < 0.5).float()
    if base == 'designed':
        u = torch.rand(N, C, H, W, generator=g)
        sign = 2 * t - 1
        x = torch.where(u < 0.4, torch.zeros_like(t), torch.where(u < 0.8, 30 * sign, -30 * sign))
    else:
        x = (2.5 * torch.randn(N, C, H, W, generator=g) + 1.5 * (2 * t - 1)).clamp(-12, 12)
    x, t = x.numpy().copy(), t.numpy().copy()
    if kind in ('absent', 'absent2'):
        t[:, 1] = 0
    if kind == 'absent2':
        x[:, 1] = (2.5 * torch.randn(N, H, W, generator=_gen('rmi-absent2', case))).clamp(-12, 12).numpy()
    if kind == 'saturated':
        x[:, 0] = 30
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t, GOUT[kind]


def designed_probs(x):
    """clamp(sigmoid(x), 1e-6, 1) of a designed logit, exact for any faithful expf: sigmoid(-30) = 9.4e-14 clamps to
    1e-6f, sigmoid(0) = 1 / (1 + 1), sigmoid(30) = 1 / (1 + 9.4e-14) = 1 / 1 (the host file proves it for fp32)"""
    assert np.isin(x, (-30.0, 0.0, 30.0)).all()
    return np.where(x == 0, F32(0.5), np.where(x > 0, F32(1.0), CLIP_MIN)).astype(F32)


def probs32(x):
    """the kernel's expression in numpy float32 (a model: numpy's expf is not the device's)"""
    x = np.asarray(x, F32)
    with np.errstate(over='ignore'):
        y = F32(1) / (F32(1) + np.exp(-x))
    return np.minimum(np.maximum(y, CLIP_MIN), F32(1))


def probs64(x):
    x = np.asarray(x, np.float64)
    return np.clip(1.0 / (1.0 + np.exp(-x)), float(CLIP_MIN), 1.0)


def pool_restate(v, g, dtype=F32, divisor=None):
    """rmi_pool_kernel (rmi.hip:47-74) on the values v [N, C, H, W]: the window's pixels inside the image added in
    row-major order in `dtype`, one division by the padded divisor.  (A pixel outside adds nothing in the kernel and
    +0 here: the same bits, the values being >= 0.)"""
    v = np.asarray(v, dtype).reshape(g.NC, g.H, g.W)
    Hq, Wq = (g.Hp - 1) * g.s + g.k, (g.Wp - 1) * g.s + g.k
    buf = np.zeros((g.NC, max(Hq, g.H + g.pad), max(Wq, g.W + g.pad)), dtype)
    buf[:, g.pad:g.pad + g.H, g.pad:g.pad + g.W] = v
    acc = np.zeros((g.NC, g.Hp, g.Wp), dtype)
    for dh in range(g.k):
        for dw in range(g.k):
            acc = acc + buf[:, dh:dh + (g.Hp - 1) * g.s + 1:g.s, dw:dw + (g.Wp - 1) * g.s + 1:g.s]
    div = (g.divisor() if divisor is None else divisor).astype(dtype)
    return (acc / div[None]).astype(dtype)


def crops(m, g, shift=0):
    """[NC, Hp, Wp] -> [NC, D, P]: crop i starts at (i / r, i % r) (rmi.hip:83, 116); shift != 0 is the mutation"""
    if shift:
        m = np.roll(m, -shift, axis=2)
    return np.stack([m[:, i // g.r:i // g.r + g.Hv, i % g.r:i % g.r + g.Wv].reshape(m.shape[0], -1)
                     for i in range(g.D)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: pooled maps
# ---------------------------------------------------------------------------------------------------------------------
def check_pool(run, x, t, g, designed, what):
    """lp: bits of torch's fp32 avg_pool2d (count_include_pad) -- the sum of a 0/1 window is an exact integer in any
    order and the one division is correctly rounded.  pp on designed logits: bits of pool_restate(designed_probs).
    pp on random logits: every element within 1/2 ulp32(ref) + (k k + 4) 2^-24 ref of the fp64 pool of the fp64
    clamped sigmoid: expf within 1 ulp (2), 1 + e (1), the division (1) -- all relative to the probability, the clamp
    being monotone --, k k - 1 adds, each relative to a partial sum <= the window's sum, and the division by the
    divisor (1); the terms are positive, so M is the reference itself."""
    tt = torch.from_numpy(np.array(t, F32))
    lp = F.avg_pool2d(tt, g.k, g.s, g.pad).numpy() if g.k > 1 else tt.numpy()
    same_bits(run['lp'], lp.reshape(g.NC, g.Hp, g.Wp), f'{what}: lp')
    if designed:
        same_bits(run['pp'], pool_restate(designed_probs(x), g), f'{what}: pp (designed)')
    else:
        ref = torch.from_numpy(pool_restate(probs64(x), g, np.float64))
        A.assert_bounded(torch.from_numpy(run['pp']), ref, ref, g.k * g.k + 4, 'f32', f'{what}: pp (random)')


# ---------------------------------------------------------------------------------------------------------------------
# stage 2: means
# ---------------------------------------------------------------------------------------------------------------------
def _exact_sums(v):
    """v [R, P] fp32 -> (q, integer sums of v 2^q as Python ints, sum|v| 2^q as Python ints): every fp32 value is an
    integer multiple of 2^-q with q = 149 at most; here q comes from the smallest nonzero magnitude"""
    v = np.asarray(v, np.float64)
    nz = np.abs(v[v != 0])
    q = 0 if nz.size == 0 else max(0, 23 - int(math.floor(math.log2(float(nz.min())))))
    assert q <= 60, 'a value too small for the exact sum'
    iv = v * 2.0 ** q                      # exact: a power-of-two scaling of an fp32 value, |iv| < 2^(q + 1)
    assert np.array_equal(iv, np.rint(iv))

    def rows(a):
        """per row the integer sum, in two int64 halves of 30 bits so that neither can overflow"""
        hi = np.floor(a / 2.0 ** 30)
        lo = a - hi * 2.0 ** 30
        return [int(h) * 2 ** 30 + int(l) for h, l in zip(hi.astype(np.int64).sum(1), lo.astype(np.int64).sum(1))]
    return q, rows(iv), rows(np.abs(iv))


def check_means(run, g, what, shift=0):
    """mean[nc][v], v < D the label crops and v >= D the probability crops (rmi.hip:76-97), from the device's own
    pp / lp.  The exact sum S of a crop is formed in integers.  Where sum|v| 2^q < 2^53 (q: every value a multiple of
    2^-q) every partial sum of any order is an integer below 2^53 times 2^-q, so the device's fp64 sum is exact and
    the mean must be the BITS of fl64(S / P) (the one rounding of the division; float(Fraction) rounds correctly).
    Elsewhere |mean - S / P| <= (P - 1) 2^-53 sum|v| / P.  Returns the number of means held to bit equality."""
    from fractions import Fraction
    exact, worst, fails = 0, 0.0, []
    for name, col0 in (('lp', 0), ('pp', g.D)):
        v = crops(run[name], g, shift).reshape(g.NC * g.D, g.P)
        q, sums, abss = _exact_sums(v)
        got = run['mean'][:, col0:col0 + g.D].reshape(-1)
        for r_, (s_, a_) in enumerate(zip(sums, abss)):
            want = Fraction(s_, g.P * 2 ** q)
            if a_ < 2 ** 53:
                exact += 1
                if not (float(want) == got[r_] and math.copysign(1, float(want)) == math.copysign(1, got[r_])):
                    fails.append(f'mean of {name} crop {r_}: got {got[r_]!r}, exactly rounded {float(want)!r}')
            else:
                bound = Fraction(g.P - 1, g.P) * Fraction(a_, 2 ** q) * Fraction(1, 2 ** 53)
                err = abs(Fraction(float(got[r_])) - want)
                worst = max(worst, float(err / bound) if bound else (0.0 if err == 0 else math.inf))
                if not err <= bound:
                    fails.append(f'mean of {name} crop {r_}: error {float(err):.3e} bound {float(bound):.3e}')
    print(f'{what}: means: {exact} of {2 * g.NC * g.D} held to the bits of the rounded exact mean; '
          f'worst bounded error {worst:.3f} of its bound' + ''.join('\n  ' + f for f in fails[:8]))
    assert not fails, f'{what}: means: {len(fails)} misses, first: {fails[0]}'
    return exact


# ---------------------------------------------------------------------------------------------------------------------
# stage 3: covariance partials
# ---------------------------------------------------------------------------------------------------------------------
def sum_chunks(part, g):
    """(Lc, S, M) [NC, D, D] fp64: the partials added chunk by chunk from 0, as rmi_solve_kernel does (rmi.hip:188-198)"""
    tot = np.zeros((g.NC, g.D, 3 * g.D))
    for ch in range(g.chunks):
        tot = tot + part[:, :, ch, :]
    return tot[:, :, :g.D].copy(), tot[:, :, g.D:2 * g.D].copy(), tot[:, :, 2 * g.D:].copy()


def check_cov(run, g, what, series=None, shift=0):
    """part[nc][i][ch][L | P | M][j] (rmi.hip:99-148) from the device's pooled maps and means.
    (a) The chunk sums of every one of the 3 D^2 entries against the long double sum of the centred products:
        |got - ref| <= (P + chunks) 2^-53 sum|term|.  Per term the device rounds the two centrings (2) and the fma (1);
        a thread adds P / (256 chunks) terms, then 6 wave steps, 4 waves and `chunks` partials: under P + chunks for
        every P >= 12 (all terms are 0 at P = 1); the long double sum's own error is 2^-11 of that.
    (b) Lc and S symmetric to the same bound.
    (c) chunk ch holds the positions [ch per, min(P, (ch + 1) per)) only: the off-diagonal entry M[0][1] (M[0][0] at
        D = 1) of every chunk against the long double sum over that range, to (per + chunks) 2^-53 sum|term|.
    series: the series to run (a) and (c) on (default all)."""
    D, P = g.D, g.P
    Lc, S, M = sum_chunks(run['part'], g)
    worst, fails = 0.0, []
    for nc in (range(g.NC) if series is None else series):
        vl = crops(run['lp'][nc:nc + 1], g, shift)[0].astype(LD) - run['mean'][nc, :D].astype(LD)[:, None]
        vp = crops(run['pp'][nc:nc + 1], g, shift)[0].astype(LD) - run['mean'][nc, D:].astype(LD)[:, None]
        al, ap = np.abs(vl), np.abs(vp)
        for got, a, b, aa, ab, nm in ((Lc[nc], vl, vl, al, al, 'Lc'), (S[nc], vp, vp, ap, ap, 'S'),
                                      (M[nc], vl, vp, al, ap, 'M')):
            ref = a @ b.T
            bound = (P + g.chunks) * U53 * (aa @ ab.T)
            err = np.abs(got.astype(LD) - ref)
            with np.errstate(invalid='ignore', divide='ignore'):
                worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0)))))
            if not (err <= bound).all():
                fails.append(f'series {nc} {nm}: worst error {float(err.max()):.3e} (bound {float(bound.max()):.3e})')
            if nm != 'M' and not (np.abs(got - got.T) <= bound.astype(np.float64)).all():
                fails.append(f'series {nc} {nm} not symmetric')
        j = 1 if D > 1 else 0
        for ch in range(g.chunks):
            p0, p1 = ch * g.per, min(P, (ch + 1) * g.per)
            term = vl[0, p0:p1] * vp[j, p0:p1]
            ref, mag = term.sum(), np.abs(term).sum()
            got = run['part'][nc, 0, ch, 2 * D + j]
            bound = (g.per + g.chunks) * U53 * mag
            if not abs(LD(got) - ref) <= bound:
                fails.append(f'series {nc} chunk {ch} [{p0}, {p1}): M[0][{j}] {got!r} vs {float(ref)!r} '
                             f'(bound {float(bound):.3e})')
    print(f'{what}: covariances: worst error {worst:.4f} of the bound (P + chunks) 2^-53 sum|term|, '
          f'P = {P}, chunks = {g.chunks}, per = {g.per}' + ''.join('\n  ' + f for f in fails[:8]))
    assert not fails, f'{what}: covariance partials: {len(fails)} misses, first: {fails[0]}'
    return Lc, S, M


# ---------------------------------------------------------------------------------------------------------------------
# stage 4: the D x D solve
# ---------------------------------------------------------------------------------------------------------------------
def _chol(a):
    """chol<D> (rmi.hip:150-165) on [D, D, n] (reads the lower triangle); NaN on a non-positive pivot"""
    D = a.shape[0]
    l = np.zeros_like(a)
    for j in range(D):
        s = a[j, j].copy()
        for k in range(j):
            s = s - l[j, k] * l[j, k]
        ok = s > 0
        d = np.where(ok, np.sqrt(np.where(ok, s, 1)), np.nan).astype(a.dtype)
        l[j, j] = d
        for i in range(j + 1, D):
            t = a[i, j].copy()
            for k in range(j):
                t = t - l[i, k] * l[j, k]
            l[i, j] = t / d
    return l


def _tri_inv(l):
    """tri_inv<D> (rmi.hip:167-179)"""
    D = l.shape[0]
    v = np.zeros_like(l)
    for j in range(D):
        v[j, j] = 1 / l[j, j]
        for i in range(j + 1, D):
            s = np.zeros_like(l[0, 0])
            for k in range(j, i):
                s = s - l[i, k] * v[k, j]
            v[i, j] = s / l[i, i]
    return v


def solve_chol(Lc, S, M, dtype, mutate=None):
    """rmi_solve_kernel (rmi.hip:181-253; losses.py:553-580 and its closed-form backward) from the summed covariances
    [n, D, D], every operation in `dtype` (np.float64: the plain Cholesky-route restatement; np.longdouble: the
    extended-precision reference).  The constants are the kernel's fp64 values.  Returns (rmi [n], Q, K [n, D, D],
    sum |log term| [n]).  mutate: 'K-transposed', 'Q-from-M' (Q = K M in place of K T)."""
    D = Lc.shape[1]
    Lc, S, M = (np.moveaxis(np.asarray(a).astype(dtype), 0, 2).copy() for a in (Lc, S, M))
    alpha, eps = dtype(np.float64(POS_ALPHA)), dtype(np.float64(DIAG_EPS))
    for i in range(D):
        S[i, i] = S[i, i] + alpha
    V = _tri_inv(_chol(S))
    Sinv = np.einsum('kan,kbn->abn', V, V)
    T = np.einsum('ikn,kjn->ijn', M, Sinv)
    Aa = Lc - np.einsum('ikn,jkn->ijn', T, M)
    for i in range(D):
        Aa[i, i] = Aa[i, i] + alpha
    L = _chol(Aa)
    dg = np.stack([L[i, i] for i in range(D)])
    logs = np.log(dg + eps)
    rmi = dtype(0.5) * (dtype(2.0) * logs.sum(0))
    V = _tri_inv(L)
    G = np.einsum('kan,kn,kbn->abn', V, dg / (dg + eps), V)
    K = np.einsum('kin,kjn->ijn', T, G)
    Q = np.einsum('ikn,kjn->ijn', K, M if mutate == 'Q-from-M' else T)
    if mutate == 'K-transposed':
        K = np.swapaxes(K, 0, 1)
    return rmi, np.moveaxis(Q, 2, 0).copy(), np.moveaxis(K, 2, 0).copy(), np.abs(logs).sum(0)


def solve_inverse(Lc, S, M):
    """the oracle's route (oracle/rmi_ref.py:57-66) in torch fp64 from the same covariances: torch.inverse (LU) of
    S + aI, torch.linalg.cholesky of A + aI, and the backward coefficients from the same inverse"""
    Lc, S, M = (torch.from_numpy(np.ascontiguousarray(a, np.float64)) for a in (Lc, S, M))
    D = Lc.shape[1]
    eye = torch.eye(D, dtype=torch.float64)
    Sinv = torch.inverse(S + eye * POS_ALPHA)
    Aa = Lc - (M @ Sinv) @ M.transpose(1, 2)
    ch = torch.linalg.cholesky(Aa + eye * POS_ALPHA)
    dg = torch.diagonal(ch, dim1=-2, dim2=-1)
    rmi = 0.5 * (2.0 * torch.sum(torch.log(dg + DIAG_EPS), dim=-1))
    Li = torch.linalg.inv(ch)
    G = Li.transpose(1, 2) @ torch.diag_embed(dg / (dg + DIAG_EPS)) @ Li
    K = Sinv @ M.transpose(1, 2) @ G
    Q = K @ M @ Sinv
    return rmi.numpy(), Q.numpy(), K.numpy()


def _rel(got, ref):
    """per series: max|got - ref| / max|ref| (0 where both are all zero), in long double"""
    n = ref.shape[0]
    d = np.abs(np.asarray(got).astype(LD) - ref).reshape(n, -1).max(1)
    m = np.abs(ref).reshape(n, -1).max(1)
    return np.where(m > 0, d / np.where(m > 0, m, 1), np.where(d > 0, np.inf, 0)).astype(np.float64)


def check_solve(run, g, cov, what):
    """rmi[nc] and coef = (Q, K) against solve_chol in long double from the device's own summed covariances.

    The error of a 9 x 9 solve follows the conditioning of S and A, not the operand sizes, so the bound is measured on
    the same covariances: e1 = the error of the fp64 Cholesky-route restatement (solve_chol in np.float64: the
    device's algorithm up to summation order and fma contraction), e2 = the error of the oracle's torch.inverse route,
    each the worst over the geometry's series -- absolute for rmi, max|d| / max|ref| per matrix for Q and K.  The
    device gets SOLVE_MARGIN = 16 x max(e1, e2) and nothing else: no floor, no derived term.
    Where M = 0 exactly (absent class, saturated channel, P = 1) Q and K must be exactly 0."""
    Lc, S, M = cov
    ref_r, ref_q, ref_k, _ = solve_chol(Lc, S, M, LD)
    c_r, c_q, c_k, _ = solve_chol(Lc, S, M, np.float64)
    i_r, i_q, i_k = solve_inverse(Lc, S, M)
    assert np.isfinite(ref_r.astype(np.float64)).all(), f'{what}: the reference solve is not finite'
    e1 = (float(np.abs(c_r.astype(LD) - ref_r).max()), float(_rel(c_q, ref_q).max()), float(_rel(c_k, ref_k).max()))
    e2 = (float(np.abs(i_r.astype(LD) - ref_r).max()), float(_rel(i_q, ref_q).max()), float(_rel(i_k, ref_k).max()))
    dev_q, dev_k = run['coef'][:, 0], run['coef'][:, 1]
    ed = (float(np.abs(run['rmi'].astype(LD) - ref_r).max()), float(_rel(dev_q, ref_q).max()),
          float(_rel(dev_k, ref_k).max()))
    bound = tuple(SOLVE_MARGIN * max(a, b) for a, b in zip(e1, e2))
    print(f'{what}: solve (rmi abs, Q rel, K rel): fp64 Cholesky route {e1[0]:.3e} {e1[1]:.3e} {e1[2]:.3e} | '
          f'torch.inverse route {e2[0]:.3e} {e2[1]:.3e} {e2[2]:.3e} | device {ed[0]:.3e} {ed[1]:.3e} {ed[2]:.3e} | '
          f'bound {bound[0]:.3e} {bound[1]:.3e} {bound[2]:.3e}')
    zero_m = np.abs(M).reshape(g.NC, -1).max(1) == 0
    assert (run['coef'][zero_m] == 0).all(), f'{what}: a series with M = 0 has nonzero coefficients'
    assert np.isfinite(run['rmi']).all() and np.isfinite(run['coef']).all(), f'{what}: solve not finite'
    for e, b, nm in zip(ed, bound, ('rmi', 'Q', 'K')):
        assert e <= b, f'{what}: {nm}: device error {e:.3e} over {SOLVE_MARGIN:g} x the host routes ({b:.3e})'
    return {'chol': e1, 'inverse': e2, 'device': ed}


# ---------------------------------------------------------------------------------------------------------------------
# stage 5: the loss scalar
# ---------------------------------------------------------------------------------------------------------------------
def loss_restate(rmi, g):
    """rmi_loss_kernel (rmi.hip:256-266): per class the rows added in order in fp64, / rows, to fp32, / float(D),
    the classes added in fp32"""
    tot = F32(0)
    for c in range(g.ncls):
        s = np.float64(0)
        for r_ in range(g.rows):
            s = s + rmi[r_ * g.ncls + c]
        tot = F32(tot + F32(F32(s / np.float64(g.rows)) / F32(g.D)))
    return F32(tot)


def check_loss(run, g, what):
    want = loss_restate(run['rmi'], g)
    print(f'{what}: loss {float(run["loss"])!r} restated from the device rmi {float(want)!r}')
    same_bits(np.asarray(run['loss'], F32).reshape(1), np.asarray(want, F32).reshape(1), f'{what}: loss')


# ---------------------------------------------------------------------------------------------------------------------
# stage 6: the pooled gradient
# ---------------------------------------------------------------------------------------------------------------------
def grad_scale(gout, g):
    """(double)(gout / (float)D) / (double)rows (rmi.hip:277)"""
    return np.float64(F32(gout) / F32(g.D)) / np.float64(g.rows)


def gp_reference(run, g, gout, shift=0):
    """rmi_grad_pooled_kernel (rmi.hip:268-304) in fp64 from the device's coef, mean, pp, lp: per crop i that contains
    the cell, c_i = scale sum_j Q_ij (p_j - muP_j) - K_ij (l_j - muL_j) over the crop's vector at its position.
    Returns (sum_i c_i, sum_i |c_i|, scale sum_i sum_j |terms|), each [NC, Hp, Wp]."""
    D = g.D
    scale = grad_scale(gout, g)
    dl = crops(run['lp'], g, shift).astype(np.float64) - run['mean'][:, :D, None]     # [NC, D, P]
    dp = crops(run['pp'], g, shift).astype(np.float64) - run['mean'][:, D:, None]
    Q, K = run['coef'][:, 0], run['coef'][:, 1]
    v = (np.einsum('nij,njp->nip', Q, dp) - np.einsum('nij,njp->nip', K, dl)) * scale
    t = (np.einsum('nij,njp->nip', np.abs(Q), np.abs(dp)) + np.einsum('nij,njp->nip', np.abs(K), np.abs(dl))) * scale
    ref, mag, terms = (np.zeros((g.NC, g.Hp, g.Wp)) for _ in range(3))
    for i in range(D):
        oy, ox = i // g.r, i % g.r
        sl = (slice(None), slice(oy, oy + g.Hv), slice(ox, ox + g.Wv))
        ref[sl] += v[:, i].reshape(g.NC, g.Hv, g.Wv)
        mag[sl] += np.abs(v[:, i]).reshape(g.NC, g.Hv, g.Wv)
        terms[sl] += t[:, i].reshape(g.NC, g.Hv, g.Wv)
    return ref, mag, np.abs(terms)


def check_gp(run, g, gout, what):
    """Every element of gp within 1/2 ulp32(ref) + (D + 1) 2^-24 M.  Each crop's value is one fp64 fma chain of 2 D
    terms, times the scale, rounded to fp32 (the roundings of the crops together: 1, against sum_i |c_i|), then at
    most D fp32 additions in crop order (D).  M = sum_i |c_i| + (2 D + 3) 2^-29 scale sum|terms| carries the fp64
    chain: 2 D fmas, two centrings and the scaling, each 2^-53 of the sum of the term magnitudes."""
    ref, mag, terms = gp_reference(run, g, gout)
    M = mag + (2 * g.D + 3) * 2.0 ** -29 * terms
    A.assert_bounded(torch.from_numpy(run['gp']), torch.from_numpy(ref), torch.from_numpy(M), g.D + 1, 'f32',
                     f'{what}: gp')
    live = float((run['gp'] != 0).mean())
    print(f'{what}: gp: {live:.3f} of the cells nonzero, max |gp| {float(np.abs(run["gp"]).max()):.3e}')


# ---------------------------------------------------------------------------------------------------------------------
# stage 7: the input gradient
# ---------------------------------------------------------------------------------------------------------------------
def check_gx(run, x, g, designed, what):
    """rmi_grad_input_kernel (rmi.hip:306-326) from the device's gp.  A pixel of a row or column no window covers
    (oy >= Hp or ox >= Wp) is exactly 0.  Designed logits: 0 at -30 (below the clamp) and at +30 ((1 - 1) y), and at
    logit 0 the bits of (gp / div) * 0.5 * 0.5 = (gp / div) / 4, one correctly rounded division.  Random logits, every
    element: the division (1), sigmoid within 4 2^-24 y (check_pool) entering y (1 - y) as |1 - 2 y| dy, the
    subtraction and the two products (3): 1/2 ulp32(ref) + 2^-24 M with M = |gp / div| y (4 |1 - 2 y| + 4 (1 - y))."""
    x3 = np.asarray(x).reshape(g.NC, g.H, g.W)
    gx = run['gx'].reshape(g.NC, g.H, g.W)
    oy, ox = (np.arange(g.H) + g.pad) // g.s, (np.arange(g.W) + g.pad) // g.s
    cov = (oy < g.Hp)[:, None] & (ox < g.Wp)[None, :]
    assert (gx[:, ~cov] == 0).all(), f'{what}: gx nonzero in an uncovered row / column'
    oyc, oxc = np.minimum(oy, g.Hp - 1), np.minimum(ox, g.Wp - 1)
    gpe = run['gp'][:, oyc[:, None], oxc[None, :]]                      # [NC, H, W]
    dive = g.divisor()[oyc[:, None], oxc[None, :]][None]
    if designed:
        sat = (np.abs(x3) == 30)
        assert (gx[sat] == 0).all(), f'{what}: gx nonzero at a saturated logit'
        want = np.where(cov[None] & (x3 == 0), (gpe / dive) * F32(0.5) * F32(0.5), F32(0)).astype(F32)
        m = np.broadcast_to(cov[None], x3.shape) & (x3 == 0)
        same_bits(gx[m], want[m], f'{what}: gx at logit 0')
        print(f'{what}: gx: {int(m.sum())} pixels at logit 0 bit-equal, {int(sat.sum())} saturated and '
              f'{int((~cov).sum()) * g.NC} uncovered exactly 0')
    else:
        y = 1.0 / (1.0 + np.exp(-x3.astype(np.float64)))
        inr = (y >= float(CLIP_MIN)) & (y <= 1.0) & cov[None]
        gpool = gpe.astype(np.float64) / dive
        ref = np.where(inr, gpool * (1.0 - y) * y, 0.0)
        M = np.where(inr, np.abs(gpool) * y * (4 * np.abs(1 - 2 * y) + 4 * (1 - y)), 0.0)
        A.assert_bounded(torch.from_numpy(gx), torch.from_numpy(ref), torch.from_numpy(M), 1, 'f32', f'{what}: gx')
        print(f'{what}: gx: every element inside 1/2 ulp + 2^-24 M; {int((~cov).sum()) * g.NC} uncovered exactly 0')


# ---------------------------------------------------------------------------------------------------------------------
# stage 8: end to end
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(case, kind):
    """(loss, grad) of oracle/rmi_ref.py; read-only"""
    from oracle import rmi_ref
    x, t, gout = operands(case, kind)
    n, c, h, w, ncls, r, k = case
    kw = dict(num_classes=ncls, radius=r, pool='avg' if k else 'none', pool_size=k or 1, pool_stride=k or 1)
    return rmi_ref.rmi_loss_and_grad(np.array(x), np.array(t), gout=gout, **kw)


def check_end_to_end(run, case, kind, what):
    """the bounds of test_hip_losses.py::test_rmi_vs_oracle: loss rtol 2e-6; gradient rtol 1e-3, atol 1e-4 max|grad|"""
    ref_l, ref_g = oracle(case, kind)
    scale = float(np.abs(ref_g).max())
    err = np.abs(run['gx'].reshape(ref_g.shape) - ref_g)
    print(f'{what}: end to end: loss {float(run["loss"])!r} oracle {float(ref_l)!r} '
          f'(rel {abs(float(run["loss"]) - float(ref_l)) / max(abs(float(ref_l)), 1e-300):.3e}); '
          f'gradient max error {float(err.max()):.3e}, max |grad| {scale:.3e}')
    np.testing.assert_allclose(float(run['loss']), float(ref_l), rtol=2e-6)
    np.testing.assert_allclose(run['gx'].reshape(ref_g.shape), ref_g, rtol=1e-3, atol=1e-4 * scale)


def closed_form_p1(g):
    """P = 1: every centred value is 0, S = A = aI, rmi = D log(sqrt(a) + 1e-8) for every series"""
    return g.D * math.log(math.sqrt(POS_ALPHA) + DIAG_EPS)


def closed_form_bound(g):
    """How far an fp64 evaluation of the closed form may lie from its value, doubled because closed_form_p1 is itself
    one: per term t = log(sqrt(a) + 1e-8) the root and the sum (2 roundings of the argument: 2 2^-53 absolute in t)
    and the logarithm within 1 ulp (2 2^-53 |t|), then D - 1 additions of partial sums below |D t| and the exact
    scalings by 2 and 1/2:  2 (2 D + (D + 1) |D t|) 2^-53."""
    return 2 * (2 * g.D + (g.D + 1) * abs(closed_form_p1(g))) * U53


def check_all(run, case, kind, what, cov_series=None):
    """every stage in order; returns the solve figures"""
    g = Geo(case)
    x, t, gout = operands(case, kind)
    designed = kind == 'designed'
    check_pool(run, x, t, g, designed, what)
    check_means(run, g, what)
    cov = check_cov(run, g, what, series=cov_series)
    fig = check_solve(run, g, cov, what)
    check_loss(run, g, what)
    check_gp(run, g, gout, what)
    check_gx(run, x, g, designed, what)
    check_end_to_end(run, case, kind, what)
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# a host model of the device (for the host file: the comparison functions must accept it and reject its mutants)
# ---------------------------------------------------------------------------------------------------------------------
def gx_model(gp, x, g, divisor):
    """rmi_grad_input_kernel in numpy float32 from a pooled gradient and a [Hp, Wp] divisor (the kernel's: g.divisor();
    the mutation: g.valid_count())"""
    oy, ox = (np.arange(g.H) + g.pad) // g.s, (np.arange(g.W) + g.pad) // g.s
    cov = (oy < g.Hp)[:, None] & (ox < g.Wp)[None, :]
    oyc, oxc = np.minimum(oy, g.Hp - 1), np.minimum(ox, g.Wp - 1)
    gpool = gp[:, oyc[:, None], oxc[None, :]] / divisor[oyc[:, None], oxc[None, :]][None]
    x3 = np.asarray(x, F32).reshape(g.NC, g.H, g.W)
    with np.errstate(over='ignore'):
        y = F32(1) / (F32(1) + np.exp(-x3))
    gx = np.where((y >= CLIP_MIN) & (y <= F32(1)) & cov[None], gpool * (F32(1) - y) * y, F32(0)).astype(F32)
    return gx.reshape(np.asarray(x).shape)


def device_model(case, kind, mutate=None):
    """What a device that follows rmi.hip returns, in the kernels' precisions (numpy's expf and summation orders in
    place of the device's), or one that carries a named fault:
      'divisor'       pooled maps divided by the number of pixels inside the image
      'crop-shift'    every crop read one column to the right (wrapping), in the means, covariances and gradient
      'chunk-leak'    chunk 0 takes the first position of chunk 1 as well (two-chunk geometries)
      'K-transposed', 'Q-from-M'   (solve_chol)"""
    g = Geo(case)
    x, t, gout = operands(case, kind)
    D = g.D
    div = g.valid_count() if mutate == 'divisor' else None
    shift = 1 if mutate == 'crop-shift' else 0
    run = {'pp': pool_restate(probs32(x), g, divisor=div), 'lp': pool_restate(t, g, divisor=div)}
    vl, vp = crops(run['lp'], g, shift).astype(np.float64), crops(run['pp'], g, shift).astype(np.float64)
    run['mean'] = np.concatenate([vl.sum(2) / g.P, vp.sum(2) / g.P], 1)
    cl, cp = vl - run['mean'][:, :D, None], vp - run['mean'][:, D:, None]
    part = np.zeros((g.NC, D, g.chunks, 3 * D))
    for ch in range(g.chunks):
        p0, p1 = ch * g.per, min(g.P, (ch + 1) * g.per)
        if mutate == 'chunk-leak' and ch == 0:
            p1 += 1
        part[:, :, ch, :D] = np.einsum('nip,njp->nij', cl[:, :, p0:p1], cl[:, :, p0:p1])
        part[:, :, ch, D:2 * D] = np.einsum('nip,njp->nij', cp[:, :, p0:p1], cp[:, :, p0:p1])
        part[:, :, ch, 2 * D:] = np.einsum('nip,njp->nij', cl[:, :, p0:p1], cp[:, :, p0:p1])
    run['part'] = part
    rmi, Q, K, _ = solve_chol(*sum_chunks(part, g), np.float64, mutate=mutate)
    run['rmi'], run['coef'] = rmi, np.stack([Q, K], 1)
    run['loss'] = loss_restate(rmi, g)
    # the pooled gradient, crop by crop in fp32
    scale = grad_scale(gout, g)
    v = (np.einsum('nij,njp->nip', Q, cp) - np.einsum('nij,njp->nip', K, cl)) * scale
    gp = np.zeros((g.NC, g.Hp, g.Wp), F32)
    for i in range(D):
        oy, ox = i // g.r, i % g.r
        if shift:
            tmp = np.zeros((g.NC, g.Hp, g.Wp), F32)
            tmp[:, oy:oy + g.Hv, ox:ox + g.Wv] = v[:, i].reshape(g.NC, g.Hv, g.Wv).astype(F32)
            gp = gp + np.roll(tmp, shift, axis=2)
        else:
            gp[:, oy:oy + g.Hv, ox:ox + g.Wv] += v[:, i].reshape(g.NC, g.Hv, g.Wv).astype(F32)
    run['gp'] = gp
    run['gx'] = gx_model(gp, x, g, g.valid_count() if mutate == 'divisor' else g.divisor())
    return run
