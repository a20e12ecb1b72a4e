"""Exact-arithmetic operands and fp64 references for the conv engine tests (test_conv_exact*.py).

Activations, weights, biases, residuals and upstream gradients are small integers (times a fixed power of two where
an activation slope or a folded BatchNorm scale needs it).  Every 16-bit product is then an exact integer, every
fp32 partial sum is exact below 2^24 in ANY summation order (split-K, tile order, k grouping), and a result of
magnitude <= 256 (bf16: 8 significant bits) / <= 2048 (fp16: 11 bits) stores without rounding.  The engine's result
must therefore EQUAL the fp64 reference cast to the storage dtype; check_exact_range is the condition that makes that
comparison legitimate and nondegenerate() the one that keeps it meaningful.  No tolerance appears anywhere.
"""
import functools
import zlib
from typing import NamedTuple

import torch
import torch.nn.functional as F

MODES = ('f32', 'bf16', 'f16')
REGIMES = ('sparse-w', 'sparse-x')
# largest magnitude m such that every integer in [-m, m] is representable in the storage dtype
STORE_BOUND = {'f32': 2 ** 24, 'bf16': 256, 'f16': 2048}
TORCH_DTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# tensors the engine always writes in fp32, whatever the compute mode
FP32_OUTPUTS = ('dW', 'db', 'dW1', 'db1', 'dW2', 'sum', 'sumsq')


class Case(NamedTuple):
    """One layer geometry.  kind: 'conv' | 'convT' | 'dw' (depthwise, cin == cout == groups).  thin scales the
    activation densities (chains, slopes and folded scales need smaller sums); seed moves every draw."""
    kind: str
    cin: int
    cout: int
    k: int
    s: int
    p: int
    d: int
    H: int
    W: int
    n: int
    bias: bool = False
    thin: float = 1.0
    seed: int = 0

    @property
    def id(self):
        return (f'{self.kind}{self.cin}-{self.cout}k{self.k}s{self.s}p{self.p}d{self.d}@{self.n}x{self.H}x{self.W}'
                + ('b' if self.bias else ''))

    def out_hw(self):
        if self.kind == 'convT':
            return (self.H - 1) * self.s - 2 * self.p + self.k, (self.W - 1) * self.s - 2 * self.p + self.k
        e = self.d * (self.k - 1) + 1
        return (self.H + 2 * self.p - e) // self.s + 1, (self.W + 2 * self.p - e) // self.s + 1


def conv(cin, cout, k, s, p, d, H, W, n, **kw):
    return Case('conv', cin, cout, k, s, p, d, H, W, n, **kw)


def convT(cin, cout, H, W, n=2, **kw):
    kw.setdefault('bias', True)
    return Case('convT', cin, cout, 4, 2, 1, 1, H, W, n, **kw)


def dw(C, k, s, p, d, H, W, n=2, **kw):
    return Case('dw', C, C, k, s, p, d, H, W, n, **kw)


def ints(shape, lo, hi, density, gen):
    """fp64 integers uniform in [lo, hi], each kept with probability `density` (otherwise 0)."""
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=gen) < density).double()
    return v


def _gen(*key):
    """a generator seeded by the key's text (stable across processes, unlike hash())"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _key(case):
    return tuple(int(v) if not isinstance(v, (str, float)) else v for v in case)


def weight_shape(case):
    if case.kind == 'dw':
        return (case.cin, 1, case.k, case.k)
    if case.kind == 'convT':
        return (case.cin, case.cout, case.k, case.k)
    return (case.cout, case.cin, case.k, case.k)


def _cover(w, gen):
    """The non-degeneracy conditions on the weights hold by construction: a tap, an input channel or an output
    channel that drew no nonzero weight (thin densities on wide layers) gets one +-1 planted."""
    def plant(dim, i):
        idx = [int(torch.randint(0, s, (1,), generator=gen)) for s in w.shape]
        if dim == 'tap':
            idx[2], idx[3] = i
        else:
            idx[dim] = i
        w[tuple(idx)] = 1.0 if int(torch.randint(0, 2, (1,), generator=gen)) else -1.0

    for dim in (0, 1):
        empty = ~(w != 0).transpose(0, dim).reshape(w.shape[dim], -1).any(1)
        for i in empty.nonzero().flatten().tolist():
            plant(dim, i)
    taps = (w != 0).any(0).any(0)
    for r, s in (~taps).nonzero().tolist():
        plant('tap', (r, s))
    return w


def _fans(case):
    """(forward contraction length per output, input-gradient contraction length per input pixel), in taps x channels"""
    rs = case.k * case.k
    if case.kind == 'dw':
        return rs, rs
    if case.kind == 'convT':
        return max(case.cin * rs // (case.s * case.s), 1), case.cout * rs
    return case.cin * rs, max(case.cout * rs // (case.s * case.s), 1)


def conv_operands(case, regime, seed=0):
    """(x, w, bias, gy) as fp64 CPU tensors (PyTorch layouts).  Two regimes, because a zero in one operand hides a
    wrong read of the other: sparse-w keeps the activations dense (x, gy in [-2, 2] at density 0.75) and thins the
    weights ([-2, 2] at min(1, 64 / max(cin R S, cout R S))); sparse-x keeps the weights dense ({-1, 0, 1} at 2/3) and
    thins each activation to min(0.75, 48 / its own contraction length).  Bias: integers in [-3, 3]."""
    assert regime in REGIMES
    rs = case.k * case.k
    oh, ow = case.out_hw()
    gw = _gen('w', regime, seed, case.seed, case.kind, case.cin, case.cout, case.k)
    ga = _gen('a', regime, seed, *_key(case))
    fin, fout = _fans(case)
    chans = (1, 1) if case.kind == 'dw' else (case.cin, case.cout)
    if regime == 'sparse-w':
        w = ints(weight_shape(case), -2, 2, min(1.0, 64.0 / max(chans[0] * rs, chans[1] * rs)), gw)
        dx_, dg_ = 0.75 * case.thin, 0.75 * case.thin
    else:
        w = ints(weight_shape(case), -1, 1, 1.0, gw)   # uniform over {-1, 0, 1}: nonzero with probability 2/3
        dx_, dg_ = min(0.75, 48.0 / fin) * case.thin, min(0.75, 48.0 / fout) * case.thin
    w = _cover(w, gw)
    x = ints((case.n, case.cin, case.H, case.W), -2, 2, dx_, ga)
    gy = ints((case.n, case.cout, oh, ow), -2, 2, dg_, ga)
    bias = ints((case.cout,), -3, 3, 1.0, gw) if case.bias else None
    return x, w, bias, gy


def apply_act(y, act):
    """act: None | 'relu' | 'relu6' | ('leaky', slope)"""
    if act is None:
        return y
    if act == 'relu':
        return F.relu(y)
    if act == 'relu6':
        return F.relu6(y)   # (gradient only where 0 < y < 6, as the engine's mask: integer data sits ON the bounds)
    if isinstance(act, tuple) and act[0] == 'leaky':
        return F.leaky_relu(y, act[1])
    raise ValueError(act)


def act_shift(act):
    """fractional bits an activation adds to integer data"""
    if isinstance(act, tuple):
        s = 0
        while act[1] * 2 ** s != int(act[1] * 2 ** s):
            s += 1
        return s
    return 0


def conv_fwd(case, x, w, bias):
    if case.kind == 'convT':
        return F.conv_transpose2d(x, w, bias, case.s, case.p)
    return F.conv2d(x, w, bias, case.s, case.p, case.d, groups=case.cin if case.kind == 'dw' else 1)


def reached(case):
    """[H, W] bool: the input positions some tap of some output reaches (a strided 1x1 skips the others)"""
    one = Case(case.kind if case.kind != 'dw' else 'conv', 1, 1, *case[3:9], 1)
    x = torch.ones(1, 1, case.H, case.W, dtype=torch.float64, requires_grad=True)
    conv_fwd(one, x, torch.ones(1, 1, case.k, case.k, dtype=torch.float64), None).sum().backward()
    return x.grad[0, 0] > 0


@functools.lru_cache(maxsize=None)
def reference(case, regime, act=None, seed=0):
    """Operands and the fp64 CPU reference of act(conv(x) + bias) and its gradients: a dict of x, w, bias, gy, y, dx,
    dW, db.  Built once per (case, regime, act) and shared by every mode and variant; treat as read-only."""
    x, w, bias, gy = conv_operands(case, regime, seed)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True) if bias is not None else None
    y = apply_act(conv_fwd(case, xr, wr, br), act)
    y.backward(gy)
    return {'x': x, 'w': w, 'bias': bias, 'gy': gy, 'y': y.detach(), 'dx': xr.grad, 'dW': wr.grad,
            'db': br.grad if br is not None else None}


def check_exact_range(ref_tensors, mode, shift=0, fp32=FP32_OUTPUTS):
    """The condition that makes torch.equal legitimate: every reference value times 2**shift is an integer of magnitude
    <= 256 where the engine stores bf16, <= 2048 where it stores fp16, <= 2^24 where it stores fp32 (f32 mode, and in
    every mode the tensors named in `fp32`: weight / bias gradients, statistics, a head=True forward)."""
    for name, t in ref_tensors.items():
        if t is None:
            continue
        v = t.double() * (2.0 ** shift)
        assert torch.equal(v, v.round()), f'{name}: not an integer multiple of 2^-{shift}'
        bound = STORE_BOUND['f32' if name in fp32 else mode]
        top = float(v.abs().max())
        assert top <= bound, f'{name}: max |v| * 2^{shift} = {top} > {bound} ({mode})'
        if name not in fp32 and mode != 'f32':
            assert torch.equal(t.to(TORCH_DTYPE[mode]).double(), t.double()), f'{name}: rounds in {mode}'


def nondegenerate(case, ref):
    """At least half of y nonzero, at least half of dx nonzero over the reached input positions, and every tap, input
    channel and output channel with a nonzero weight."""
    y, dx, w = ref['y'], ref['dx'], ref['w']
    share = float((y != 0).double().mean())
    assert share >= 0.5, f'y: nonzero share {share:.3f}'
    m = reached(case)
    share = float((dx != 0)[:, :, m].double().mean())
    assert share >= 0.5, f'dx: nonzero share over reached positions {share:.3f}'
    nz = w != 0
    assert bool(nz.any(0).any(0).all()), 'a tap without a nonzero weight'
    for dim in (0, 1):
        assert bool(nz.transpose(0, dim).reshape(w.shape[dim], -1).any(1).all()), 'a channel without a nonzero weight'


def assert_exact(got, want, what):
    """torch.equal(engine result, fp64 reference cast to the engine's dtype); on a mismatch the count and the first
    few (index, got, want) are printed."""
    g = got.detach().cpu()
    w = want.to(g.dtype)
    assert g.shape == w.shape, f'{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}'
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        rows = [f'  {tuple(i.tolist())}: got {float(g[tuple(i.tolist())])} want {float(w[tuple(i.tolist())])}'
                for i in bad[:8]]
        print(f'{what}: {bad.shape[0]} of {g.numel()} elements differ (n, c, h, w / index, got, want)\n'
              + '\n'.join(rows))
    assert torch.equal(g, w), f'{what}: differs from the fp64 reference (details in the captured output)'


def clear_caches():
    for f in (reference, chain_reference, join_reference, vcat_reference, fold_reference):
        f.cache_clear()


def outputs(ref, names=('y', 'dx', 'dW', 'db')):
    """the reference tensors the engine produces, keyed as check_exact_range names them"""
    return {k: ref[k] for k in names if ref.get(k) is not None}


# ---------------------------------------------------------------------------------------------------------------------
# the case table (shared by the GPU file and the host file that keeps it honest)
# ---------------------------------------------------------------------------------------------------------------------
CONV_CASES = [conv(*c) for c in [
    # cin, cout, k, stride, pad, dil, H, W, N   (test_hip_layers.CONV_CASES)
    (8, 16, 3, 1, 1, 1, 12, 10, 2), (16, 64, 1, 1, 0, 1, 9, 9, 2), (64, 32, 1, 2, 0, 1, 10, 11, 2),
    (16, 32, 3, 2, 1, 1, 13, 12, 2), (3, 64, 7, 2, 3, 1, 23, 22, 2), (32, 16, 3, 1, 2, 2, 11, 11, 1),
    (24, 40, 3, 1, 1, 1, 7, 9, 3), (128, 128, 3, 1, 1, 1, 8, 8, 2)]]

# chosen against the engine's tile sizes: 128 x 64 and 64 x 64 output tiles, 64-deep k-tiles, 8-channel vectors
RAGGED = [conv(64, 128, 3, 1, 1, 1, 19, 22, 2), conv(128, 64, 1, 1, 0, 1, 17, 20, 2),
          conv(192, 256, 3, 1, 1, 1, 9, 12, 2), conv(256, 200, 1, 1, 0, 1, 23, 26, 2),
          conv(128, 256, 1, 2, 0, 1, 18, 21, 2), conv(32, 64, 3, 2, 0, 1, 26, 29, 2)]
GENERAL_K = [conv(8, 48, 3, 1, 1, 1, 17, 20, 2), conv(48, 50, 3, 1, 1, 1, 15, 18, 2),
             conv(50, 28, 1, 1, 0, 1, 19, 22, 2)]
VPAD = [conv(240, 120, 3, 1, 1, 1, 11, 14, 2)]
DILATED = [conv(64, 64, 3, 1, 2, 2, 13, 15, 2), conv(64, 64, 3, 1, 4, 4, 13, 15, 2)]
HALO = [conv(64, 64, 3, 1, 1, 1, 8, 64, 2), conv(32, 32, 3, 1, 1, 1, 8, 64, 2), conv(64, 192, 3, 1, 1, 1, 4, 128, 2),
        conv(64, 64, 3, 1, 1, 1, 16, 16, 2), conv(64, 64, 3, 1, 1, 1, 32, 32, 2)]
POINTWISE = [conv(64, 256, 1, 1, 0, 1, 150, 153, 2), conv(128, 128, 1, 1, 0, 1, 50, 31, 2)]
SPLIT_K = [conv(512, 64, 3, 1, 1, 1, 4, 4, 2), conv(176, 28, 3, 1, 1, 1, 16, 16, 2),
           conv(2048, 128, 3, 1, 1, 1, 8, 8, 1)]
STEM = [conv(3, 64, 7, 2, 3, 1, 38, 256, 2), conv(3, 64, 3, 2, 1, 1, 33, 512, 2)]
CONVT = [convT(16, 8, 5, 6), convT(128, 64, 8, 7), convT(256, 128, 8, 9)]
DEPTHWISE = [dw(24, 3, 1, 1, 1, 9, 11), dw(32, 3, 2, 1, 1, 13, 12), dw(16, 5, 1, 2, 1, 7, 8),
             dw(40, 3, 1, 2, 2, 10, 9), dw(12, 3, 2, 1, 1, 9, 9)]
AUTO_CASES = CONV_CASES + RAGGED + GENERAL_K + VPAD + DILATED + HALO + POINTWISE + SPLIT_K

# one case of each family, run on every forced variant
VARIANT_CASES = [RAGGED[0], GENERAL_K[1], VPAD[0], HALO[0], HALO[4], HALO[3], POINTWISE[1], RAGGED[4], CONVT[1]]
# (knob, value) -> the cases it can change
KNOB_CASES = [
    (8, -1, [RAGGED[0], GENERAL_K[1], RAGGED[4], HALO[0], CONVT[1]]),      # register-staged weight gradient
    (11, -1, [HALO[0], HALO[1], HALO[4]]),                                # halo kernels off (fwd, dgrad, wgrad)
    (13, -1, POINTWISE[1:] + [RAGGED[1]]),                                # pointwise kernels off
    (14, -1, SPLIT_K), (14, 2, SPLIT_K + [RAGGED[2]]), (14, 4, SPLIT_K + [RAGGED[2]]), (14, 8, SPLIT_K),
    (7, -1, [RAGGED[0], GENERAL_K[1], VPAD[0], POINTWISE[1], CONVT[1]]),  # LDS-staged epilogue off
    (16, -1, [HALO[3], HALO[4]]),                                         # 64-wide halo tiles on 16^2 / 32^2 maps
]
# (knob that switches a kernel family off, a variant of that family, a case it runs): the first row's geometry is what
# test_conv_knobs caught -- a cached pointwise variant with knob 13 = -1 failed the launch (SSSEG_EUNSUPPORTED)
POINTWISE_SMALL = conv(64, 256, 1, 1, 0, 1, 9, 13, 2)
STALE_ROWS = [(13, 27, RAGGED[1]), (13, 26, POINTWISE_SMALL), (11, 24, HALO[0]), (11, 25, HALO[1]),
              (15, 28, HALO[0])]
MERGED_CASES = [RAGGED[0], GENERAL_K[1], HALO[0], CONVT[1]]   # defer_wgrad + flush_wgrad, batches (2, 3)

LEAKY = ('leaky', 0.25)
ACT_CASES = [conv(24, 40, 3, 1, 1, 1, 7, 9, 3, bias=True), conv(64, 128, 3, 1, 1, 1, 19, 22, 2, bias=True)]
ACTS = ('relu', 'relu6', LEAKY)


def act_case(case, act):
    """a slope of 2^-2 costs two of the storage format's bits: thinner activations keep 4 y within the bound"""
    return case._replace(thin=0.25) if isinstance(act, tuple) else case


# ---------------------------------------------------------------------------------------------------------------------
# composites: fp64 references of the unfused math
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_ACTS = ('relu', LEAKY)


@functools.lru_cache(maxsize=None)
def chain_reference(act, regime):
    """Conv4x4/s2 + act feeding one Conv4x4/s2 (the discriminator's first two layers): x 2 x 8 x 34 x 30, 8 -> 32 ->
    48, both with bias.  The second layer's weights are sparser so the chain stays in range."""
    c1 = conv(8, 32, 4, 2, 1, 1, 34, 30, 2, bias=True, thin=0.4 if isinstance(act, tuple) else 0.6)
    x, w1, b1, _ = conv_operands(c1, regime, 3)
    g = _gen('chain', regime, str(act))
    w2 = _cover(ints((48, 32, 4, 4), -1, 1, 0.03, g), g)
    b2 = ints((48,), -3, 3, 1.0, g)
    xr = x.clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    h = apply_act(F.conv2d(xr, p[0], p[1], 2, 1), act)
    h.retain_grad()
    y = F.conv2d(h, p[2], p[3], 2, 1)
    gy = ints(y.shape, -2, 2, 0.25, g)
    y.backward(gy)
    return {'x': x, 'w1': w1, 'b1': b1, 'w2': w2, 'b2': b2, 'gy': gy, 'h': h.detach(), 'y': y.detach(),
            'dh': h.grad, 'dx': xr.grad, 'dW1': p[0].grad, 'db1': p[1].grad, 'dW2': p[2].grad}


JOIN_CASES = [(64, 16, 9, 7), (64, 16, 16, 16), (256, 64, 9, 7), (256, 64, 16, 16)]   # cin, cout, H, W (N = 2)


@functools.lru_cache(maxsize=None)
def join_reference(cin, cout, H, W, regime):
    """The residual join's input gradient: relu'(z) * (dgrad_1x1(gy) + add), z >= 0 the join's output."""
    c = conv(cin, cout, 1, 1, 0, 1, H, W, 2)
    z, w, _, gy = conv_operands(c, regime, 5)
    g = _gen('join', cin, cout, H, W, regime)
    z = ints(z.shape, 0, 2, 0.75, g)   # a ReLU output: half of it closed, whatever the regime
    add = ints(z.shape, -3, 3, 0.75, g)
    d = torch.nn.grad.conv2d_input(z.shape, w, gy) + add
    return {'z': z, 'w': w, 'gy': gy, 'add': add, 'dx': d * (z > 0)}


VCAT_CASES = [(64, 64, 9, 12), (128, 64, 16, 16)]   # ca, cb, H, W (N = 2, 3x3 to 64 channels)


@functools.lru_cache(maxsize=None)
def vcat_reference(ca, cb, H, W, regime):
    c = conv(ca + cb, 64, 3, 1, 1, 1, H, W, 2)
    x, w, _, gy = conv_operands(c, regime, 7)
    r = reference(c, regime, None, 7)
    return {'a': x[:, :ca], 'b': x[:, ca:], 'w': w, 'gy': gy, 'y': r['y'], 'da': r['dx'][:, :ca],
            'db_part': r['dx'][:, ca:], 'dW': r['dW']}


FOLD_CASES = [conv(24, 20, 3, 1, 1, 1, 10, 9, 2, thin=0.5), conv(64, 128, 3, 1, 1, 1, 11, 13, 2, bias=True, thin=0.5),
              conv(64, 256, 1, 1, 0, 1, 21, 20, 2, thin=0.5)]


@functools.lru_cache(maxsize=None)
def fold_reference(case, regime):
    """relu(bn_eval(conv(x)) + residual) with an exactly representable fold: eps = 0, running_var in {0.25, 1, 4},
    gamma a power of two in [0.5, 2] (drawn so that gamma / sqrt(var) stays in {0.5, 1, 2}), integer running_mean, beta
    and residual.  Every value is a multiple of 0.5 (shift = 1)."""
    x, w, bias, gy = conv_operands(case, regime, 9)
    g = _gen('fold', *_key(case), regime)
    C = case.cout
    std = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    gamma = (scale * std).clamp(0.5, 2.0)
    mean, beta = ints((C,), -2, 2, 1.0, g), ints((C,), -3, 3, 1.0, g)
    oh, ow = case.out_hw()
    res = ints((case.n, C, oh, ow), -3, 3, 0.75, g)
    xr, rr = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    v = lambda t: t.view(1, C, 1, 1)  # noqa: E731  (eps = 0: written out, F.batch_norm refuses it)
    z = (F.conv2d(xr, wr, bias, case.s, case.p, case.d) - v(mean)) / v(std) * v(gamma) + v(beta)
    y = F.relu(z + rr)
    y.backward(gy)
    return {'x': x, 'w': w, 'bias': bias, 'gy': gy, 'res': res, 'gamma': gamma, 'beta': beta, 'mean': mean,
            'var': std * std, 'scale': gamma / std, 'y': y.detach(), 'dx': xr.grad, 'dres': rr.grad, 'dW': wr.grad}


STATS_CASES = [RAGGED[0], GENERAL_K[1], RAGGED[4], HALO[0], POINTWISE[1], CONVT[1]._replace(bias=False),
               CONV_CASES[0]]


def stats_reference(case, regime):
    r = reference(case, regime)
    return {'sum': r['y'].sum((0, 2, 3)), 'sumsq': (r['y'] * r['y']).sum((0, 2, 3))}
