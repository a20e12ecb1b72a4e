"""Operands and fp64 references for the kernels between the convolutions (test_aux_exact*.py): BatchNorm, the pools,
the n-ary add, concat / copy, the activation backward, the NHWC bilinear resize, dropout and the attention blend.

Tier A (exact).  The operands are small dyadic rationals chosen so that EVERY intermediate a kernel forms is exactly
representable in fp32 (in any summation order) and every stored result in the storage dtype: the kernel's result must
EQUAL the fp64 reference cast to the storage dtype (exact.assert_exact).  exact.check_exact_range is the condition
that makes the comparison legitimate, nondegenerate() the one that keeps it meaningful; test_aux_exact_host.py proves
both for every case without a GPU.

Tier B (bounded per element).  Where the arithmetic cannot be exact (a divisor of 9, 1/143, a random invstd, a
sigmoid) EVERY element is held to
    |got - ref| <= 1/2 ulp_store(ref) + k 2^-24 M
with ref the fp64 result on the storage-rounded inputs, M the sum of the magnitudes of the terms that form the
element and k the number of fp32 roundings of the kernel's expression (plus the number of terms of a sum), counted
from the kernel source and stated in the docstring of each Tier B reference (or of its *_k helper).  No element is
excluded and no mean is taken.

All tensors here are fp64 CPU tensors in PyTorch's NCHW layout; the references are built once per case
(functools.lru_cache) and shared by every test: treat them as read-only.
"""
import functools
import math

import torch
import torch.nn.functional as F

from exact import MODES, STORE_BOUND, TORCH_DTYPE, _gen, apply_act, check_exact_range, ints  # noqa: F401

LEAKY = ('leaky', 0.25)
U24 = 2.0 ** -24   # one fp32 rounding, relative to the rounded value


def chans(C, mode):
    """The channel counts are chosen against 8-element (16-bit) vectors; fp32 vectors hold 4, so f32 runs C / 2."""
    return C // 2 if mode == 'f32' else C


def nondegenerate(t, what, share=0.5, distinct=3):
    """At least `share` of t nonzero, and every channel (dim 1) carrying at least `distinct` different values:
    all-equal data hides a wrong read."""
    got = float((t != 0).double().mean())
    assert got >= share, f'{what}: nonzero share {got:.3f} < {share}'
    if t.dim() >= 2:
        rows = t.transpose(0, 1).reshape(t.shape[1], -1)
        srt = rows.sort(1).values
        n = 1 + (srt[:, 1:] != srt[:, :-1]).sum(1)
        assert int(n.min()) >= min(distinct, rows.shape[1]), f'{what}: a channel with {int(n.min())} distinct values'


def nz(t):
    """zeros replaced by ones: a gradient that is nonzero everywhere"""
    return torch.where(t == 0, torch.ones_like(t), t)


def clear_caches():
    for f in (bn_train_reference, bn_eval_reference, pool_reference, gap_reference, add_reference, cat_reference,
              crop_reference, act_bwd_reference, resize_reference, bn_train_random, avgpool3_random, gap_random,
              resize_random, att_blend_random):
        f.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: BatchNorm in training mode with designed statistics
# ---------------------------------------------------------------------------------------------------------------------
# one 16-pixel group: mean 0, mean square 1
MULTISET = (-2,) + (-1,) * 4 + (0,) * 6 + (1,) * 4 + (2,)
BN_FLAGS = ((False, False), (True, False), (True, True), (False, True))   # (relu, residual)
# C (16-bit modes; f32 runs C / 2) against layout_for / wide_ok of csrc/bn.hip:
#   12: one 16-byte chunk half padding; 24: nch 3, ppb 85, one idle thread; 200: 25 chunks in one block row;
#   264: cblocks 2 with one chunk in the last block; 1032: cblocks 5 at the small-map cap
BN_C = (12, 24, 200, 264, 1032)
BN_MAP = (2, 8, 17)          # P = 272: a multiple of 16 but not of ppb * U, so the pl tail and the u tail both run
BN_BIG = (16, (1, 256, 256))  # P = 65536: the 256-chunk layout
BN_MOMENTUM = 0.25
BN_CASES = [(C, BN_MAP) for C in BN_C] + [BN_BIG]
BN_EVAL_CASES = [(C, BN_MAP) for C in BN_C]


def bn_id(C, nhw):
    return f'C{C}@{nhw[0]}x{nhw[1]}x{nhw[2]}'


def _balanced(C, P, g):
    """[C, P]: per channel a random permutation of P / 16 copies of MULTISET"""
    assert P % 16 == 0
    base = torch.tensor(MULTISET, dtype=torch.float64).repeat(P // 16)
    return base[torch.rand(C, P, generator=g).argsort(1)]


def _half_live(r, g):
    """[C, P] bool: a live set of exactly P / 2 pixels per channel with sum r = 0 and sum r^2 = P / 2 over it, so
    the backward means over the live set are (a / 2, b / 2).  Whole 16-pixel groups cannot give a power-of-two share
    of P = 272 = 16 * 17 pixels, so the set is drawn by value instead: with G = P / 16 and p = G // 2 it takes p
    pixels of each of r = -2, 2, 4 G - 4 p of each of r = -1, 1 and 6 p of r = 0 (2 p + 2 (4 G - 4 p) + 6 p = 8 G
    pixels, sum r^2 = 8 p + 8 G - 8 p = 8 G)."""
    C, P = r.shape
    G = P // 16
    p = G // 2
    take = {-2: p, 2: p, -1: 4 * G - 4 * p, 1: 4 * G - 4 * p, 0: 6 * p}
    score = torch.rand(C, P, generator=g)
    live = torch.zeros(C, P, dtype=torch.bool)
    for v, n in take.items():
        idx = torch.where(r == v, score, torch.full_like(score, 2.0)).argsort(1)[:, :n]
        live.scatter_(1, idx, torch.ones_like(idx, dtype=torch.bool))
    return live


def _paired_noise(r, live, g):
    """[C, P] integers in [-3, 3], +k and -k on random pairs of live pixels that share the same r, 0 elsewhere:
    sum n = sum n r = 0 over the live set"""
    C, P = r.shape
    key = torch.where(live, r + 2.0, torch.full_like(r, 9.0)) * 2.0 + torch.rand(C, P, generator=g)
    order = key.argsort(1)   # live pixels first, grouped by r, random inside a group
    first, second = order[:, 0:P - 1:2], order[:, 1:P:2]
    same = (r.gather(1, first) == r.gather(1, second)) & live.gather(1, first) & live.gather(1, second)
    k = ints(first.shape, -3, 3, 1.0, g) * same.double()
    n = torch.zeros_like(r)
    n.scatter_(1, first, k)
    n.scatter_(1, second, -k)
    return n


def _nchw(t, nhw):
    """[C, P] -> [N, C, H, W] (P runs over n, h, w in that order, like the NHWC pixel index)"""
    n, h, w = nhw
    return t.view(t.shape[0], n, h, w).permute(1, 0, 2, 3).contiguous()


def _cp(t):
    """[N, C, H, W] -> [C, P]"""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


@functools.lru_cache(maxsize=None)
def bn_train_reference(C, nhw, relu, residual):
    """act(bn_train(x) [+ res]) and its backward with eps = 0 on designed statistics.

    x = m + s r with r a balanced permutation (mean 0, mean square 1): mean = m, invstd = 1 / s, x_hat = r exactly.
    gy = a + b r + n on the live set with n paired noise, so sum dy = L a + b sum r, sum dy x_hat = a sum r + b sum r^2
    over the L live pixels.  relu without residual: beta = 0, the live set is r > 0 (5 P / 16 pixels, sum r = 6 P / 16,
    sum r^2 = 8 P / 16).  relu with residual: the residual drives the mask (_half_live; +7..10 on live pixels, -10..-7
    on closed ones, |gamma r + beta| <= 6).  Dead pixels carry a random gradient that the mask must remove.
    The backward is the plain formula dx = gamma invstd (dyr - mean(dyr) - x_hat mean(dyr x_hat)) written out, each
    step exact in fp64 (the host file checks it against fp64 autograd)."""
    g = _gen('bn-train', C, nhw, relu, residual)
    n_, h_, w_ = nhw
    P = n_ * h_ * w_
    def pick(vals, k):
        return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (k,), generator=g)]
    m, s = ints((C,), -2, 2, 1.0, g), pick([1.0, 2.0, 4.0], C)
    gamma = pick([0.5, 1.0, 2.0], C)
    beta = ints((C,), -2, 2, 1.0, g) if not (relu and not residual) else torch.zeros(C, dtype=torch.float64)
    r = _balanced(C, P, g)
    x = m[:, None] + s[:, None] * r
    col = lambda v: v[:, None]  # noqa: E731
    res = None
    if residual and relu:
        live = _half_live(r, g)
        mag = ints((C, P), 7, 10, 1.0, g)
        res = torch.where(live, mag, -mag)
    elif residual:
        live = torch.ones(C, P, dtype=torch.bool)
        res = ints((C, P), -3, 3, 1.0, g)
    elif relu:
        live = r > 0
    else:
        live = torch.ones(C, P, dtype=torch.bool)
    a, b = 2 * ints((C,), -1, 1, 1.0, g), 2 * ints((C,), -1, 1, 1.0, g)
    gy = torch.where(live, col(a) + col(b) * r + _paired_noise(r, live, g), ints((C, P), -3, 3, 1.0, g))

    # the reference, written out (F.batch_norm refuses eps = 0)
    mean = x.sum(1) / P
    var = (x * x).sum(1) / P - mean * mean
    invstd = 1.0 / var.sqrt()
    xh = (x - col(mean)) * col(invstd)
    z = col(gamma) * xh + col(beta) + (res if res is not None else 0.0)
    y = F.relu(z) if relu else z
    dyr = gy * (z > 0) if relu else gy
    mdy, mdyx = dyr.sum(1) / P, (dyr * xh).sum(1) / P
    dx = col(gamma * invstd) * (dyr - col(mdy) - xh * col(mdyx))
    rm0, rv0 = ints((C,), -3, 3, 1.0, g), pick([0.5, 1.0, 2.0], C)
    out = {'x': _nchw(x, nhw), 'gy': _nchw(gy, nhw), 'res': _nchw(res, nhw) if res is not None else None,
           'gamma': gamma, 'beta': beta, 'm': m, 's': s, 'a': a, 'b': b, 'r': r, 'live': live, 'z': _nchw(z, nhw),
           'mean': mean, 'invstd': invstd, 'rm0': rm0, 'rv0': rv0,
           'y': _nchw(y, nhw), 'dx': _nchw(dx, nhw), 'dres': _nchw(dyr, nhw) if residual else None,
           'dgamma': (dyr * xh).sum(1), 'dbeta': dyr.sum(1), 'mdy': mdy, 'mdyx': mdyx,
           'running_mean': (1 - BN_MOMENTUM) * rm0 + BN_MOMENTUM * mean,
           'running_var': (1 - BN_MOMENTUM) * rv0 + BN_MOMENTUM * var * P / (P - 1)}
    return out


BN_FP32 = ('dgamma', 'dbeta', 'running_mean')


def bn_train_check_range(ref, mode):
    """check_exact_range for every output of a bn_train_reference.  y is a multiple of 1/2 (gamma >= 1/2).  dx is
    gamma / s times a multiple of 1/8 (the backward means over the r > 0 live set are multiples of 1/8): it is checked
    channel-wise, divided by its power-of-two factor, at shift 3 -- a power-of-two factor changes neither the
    significand nor, at these magnitudes, the representability."""
    check_exact_range({'y': ref['y'], 'x': ref['x'], 'gy': ref['gy'], 'res': ref['res'], 'dres': ref['dres']}, mode, 1)
    gi = (ref['gamma'] * ref['invstd']).view(1, -1, 1, 1)
    check_exact_range({'dx/gi': ref['dx'] / gi}, mode, 3)
    check_exact_range({k: ref[k] for k in BN_FP32}, mode, 2, fp32=BN_FP32)
    if mode != 'f32':
        dx = ref['dx']
        assert torch.equal(dx.to(TORCH_DTYPE[mode]).double(), dx), f'dx rounds in {mode}'


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: BatchNorm in eval mode (bn_act and the folded-BN backward entry points)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_eval_reference(C, nhw, relu, residual):
    """act((x - mean) gamma / sigma + beta [+ res]) with an exactly representable fold, as exact.fold_reference:
    eps = 0, running_var in {0.25, 1, 4}, gamma / sigma in {0.5, 1, 2}, integer mean, beta, residual.  Every value is
    a multiple of 1/2.  The gradients are those of the plain expression (fp64 autograd)."""
    g = _gen('bn-eval', C, nhw, relu, residual)
    n_, h_, w_ = nhw
    def pick(vals):
        return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (C,), generator=g)]
    std, scale = pick([0.5, 1.0, 2.0]), pick([0.5, 1.0, 2.0])
    gamma = scale * std
    mean, beta = ints((C,), -2, 2, 1.0, g), ints((C,), -3, 3, 1.0, g)
    x = ints((n_, C, h_, w_), -3, 3, 1.0, g)
    res = ints(x.shape, -3, 3, 0.75, g) if residual else None
    gy = nz(ints(x.shape, -2, 2, 1.0, g))
    v = lambda t: t.view(1, C, 1, 1)  # noqa: E731
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if residual else None
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = (xr - v(mean)) / v(std) * v(gr) + v(br) + (rr if residual else 0.0)
    y = F.relu(z) if relu else z
    y.backward(gy)
    return {'x': x, 'res': res, 'gy': gy, 'gamma': gamma, 'beta': beta, 'mean': mean, 'var': std * std, 'std': std,
            'scale': scale, 'shift': beta - mean * scale, 'invstd': 1.0 / std, 'z': z.detach(), 'y': y.detach(),
            'dx': xr.grad, 'dres': rr.grad if residual else None, 'dgamma': gr.grad, 'dbeta': br.grad}


BN_EVAL_FP32 = ('dgamma', 'dbeta')


def bn_eval_check_range(ref, mode):
    check_exact_range({k: ref[k] for k in ('x', 'res', 'gy', 'y', 'dx', 'dres')}, mode, 1)
    check_exact_range({k: ref[k] for k in BN_EVAL_FP32}, mode, 1, fp32=BN_EVAL_FP32)


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: pools
# ---------------------------------------------------------------------------------------------------------------------
# (kind, k, s, p, ceil) x C x (H, W); odd H and W hang a window over each border
MAXPOOLS = (('max', 3, 2, 1, False), ('max', 2, 2, 0, True))
AVGPOOL = ('avg', 2, 2, 0, False)
POOL_CASES = ([(op, C, hw) for op in MAXPOOLS for C in (16, 24) for hw in ((9, 7), (13, 11))]
              + [(AVGPOOL, C, hw) for C in (16, 24) for hw in ((9, 7), (8, 8))])


def pool_id(op, C, hw):
    return f'{op[0]}{op[1]}s{op[2]}p{op[3]}{"c" if op[4] else ""}-C{C}@{hw[0]}x{hw[1]}'


@functools.lru_cache(maxsize=None)
def pool_reference(op, C, hw):
    """F.max_pool2d on tie-heavy integers in [-4, 4] (PyTorch's CPU kernel and ours both keep the FIRST maximum in
    (kh, kw) order) or F.avg_pool2d(2, 2) (divisor 4: multiples of 1/4); `add` is an integer tensor for the
    residual-added max-pool backward (dx + add)."""
    kind, k, s, p, ceil = op
    g = _gen('pool', op, C, hw)
    x = ints((2, C) + tuple(hw), -4, 4, 1.0, g) if kind == 'max' else ints((2, C) + tuple(hw), -2, 2, 1.0, g)
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, p, ceil_mode=ceil) if kind == 'max' else F.avg_pool2d(xr, k, s, p)
    gy = ints(y.shape, -2, 2, 0.75, g)
    y.backward(gy)
    add = ints(x.shape, -3, 3, 0.75, g)
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad, 'add': add, 'dx_add': xr.grad + add}


# (C, H, W, what): HW = 64 one split, HW = 1024 four splits, C = 520 the second channel block of 64 chunks in bf16
GAP_CASES = ((24, 8, 8), (16, 32, 32), (520, 8, 8))


@functools.lru_cache(maxsize=None)
def gap_reference(C, H, W):
    """AdaptiveAvgPool2d(1) with HW a power of two on sparse {-1, 0, 1} data: the sum is an integer of magnitude well
    under 256 and 1 / HW is exact, so y = k / HW and dx = gy / HW exactly."""
    g = _gen('gap', C, H, W)
    x = ints((2, C, H, W), -1, 1, 0.75 if H * W <= 64 else 0.25, g)
    gy = ints((2, C, 1, 1), -2, 2, 1.0, g)
    gy = torch.where(gy == 0, torch.ones_like(gy), gy)
    xr = x.clone().requires_grad_(True)
    y = F.adaptive_avg_pool2d(xr, 1)
    y.backward(gy)
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad}


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: n-ary add, concat, crop, copies, activation backward
# ---------------------------------------------------------------------------------------------------------------------
ADD_N = (2, 3, 8)
ADD_ACTS = (None, 'relu', LEAKY)
ADD_SHAPE = (2, 24, 7, 9)   # 3024 elements: 378 16-bit chunks / 756 fp32 chunks, a partial last workgroup of 256


@functools.lru_cache(maxsize=None)
def add_reference(n, act):
    g = _gen('add', n, str(act))
    xs = [ints(ADD_SHAPE, -2, 2, 0.75, g) for _ in range(n)]
    gy = nz(ints(ADD_SHAPE, -2, 2, 1.0, g))
    xr = [t.clone().requires_grad_(True) for t in xs]
    y = apply_act(sum(xr[1:], xr[0]), act)
    y.backward(gy)
    assert all(torch.equal(t.grad, xr[0].grad) for t in xr)
    return {'xs': xs, 'gy': gy, 'y': y.detach(), 'dx': xr[0].grad}


CAT_WIDTHS = ((10, 6, 14), (14, 18, 10, 24))   # HarDNet's ragged growth-rate widths
CAT_MAP = (2, 7, 9)


@functools.lru_cache(maxsize=None)
def cat_reference(widths):
    g = _gen('cat', widths)
    n, h, w = CAT_MAP
    xs = [ints((n, c, h, w), -3, 3, 0.9, g) for c in widths]
    gy = ints((n, sum(widths), h, w), -3, 3, 0.9, g)
    return {'xs': xs, 'gy': gy, 'y': torch.cat(xs, 1), 'dxs': list(gy.split(list(widths), 1))}


CROP_CASES = ((16, 24, (9, 11), (7, 8)), (10, 6, (8, 8), (8, 8)), (24, 16, (6, 7), (10, 9)))   # ca, cb, a's map, b's


@functools.lru_cache(maxsize=None)
def crop_reference(ca, cb, hwa, hwb):
    """torch.cat of a and b along channels, the larger map center-cropped to the smaller in each dimension"""
    g = _gen('crop', ca, cb, hwa, hwb)
    a, b = ints((2, ca) + tuple(hwa), -3, 3, 0.9, g), ints((2, cb) + tuple(hwb), -3, 3, 0.9, g)
    H, W = min(hwa[0], hwb[0]), min(hwa[1], hwb[1])
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def crop(t):
        oy, ox = (t.shape[2] - H) // 2, (t.shape[3] - W) // 2
        return t[:, :, oy:oy + H, ox:ox + W]
    y = torch.cat((crop(ar), crop(br)), 1)
    gy = ints(y.shape, -3, 3, 0.9, g)
    y.backward(gy)
    return {'a': a, 'b': b, 'gy': gy, 'y': y.detach(), 'da': ar.grad, 'db': br.grad}


ACT_BWD = (None, 'relu', 'relu6', LEAKY)
ACT_BWD_N = 3001 * 8   # an odd number of 16-byte chunks, a partial last workgroup


@functools.lru_cache(maxsize=None)
def act_bwd_reference(act):
    """gx = gy act'(y) from the OUTPUT y, integers in [-2, 8] so that the boundary points 0 and 6 are hit: the
    engine's masks are strict there (ReLU passes y > 0, ReLU6 0 < y < 6, LeakyReLU 1 for y > 0 and the slope else)."""
    g = _gen('act-bwd', str(act))
    y = ints((ACT_BWD_N,), -2, 8, 1.0, g)
    gy = ints((ACT_BWD_N,), -2, 2, 1.0, g)
    gy = torch.where(gy == 0, torch.ones_like(gy), gy)
    if act is None:
        gx = gy.clone()
    elif act == 'relu':
        gx = gy * (y > 0)
    elif act == 'relu6':
        gx = gy * ((y > 0) & (y < 6))
    else:
        gx = torch.where(y > 0, gy, gy * act[1])
    return {'y': y, 'gy': gy, 'gx': gx}


# ---------------------------------------------------------------------------------------------------------------------
# Tier A: NHWC bilinear resize with dyadic weights
# ---------------------------------------------------------------------------------------------------------------------
def _resize_cases():
    out = []
    for C in (8, 24):
        for h, w in ((5, 7), (9, 6)):
            out += [(C, (h, w), (2 * h, 2 * w), False), (C, (h, w), (4 * h, 4 * w), False),
                    (C, (2 * h, 2 * w), (h, w), False)]   # 2x down ONTO the 5x7 / 9x6 maps (in / out = 2 exactly)
    out.append((8, (5, 9), (9, 17), True))   # 2^k + 1 -> 2^(k+1) + 1: weights 0 and 1/2
    return out


RESIZE_CASES = _resize_cases()
RESIZE_SHIFT = 6   # per-axis weights are multiples of 1/8


def resize_id(C, hw, size, ac):
    return f'C{C}@{hw[0]}x{hw[1]}-{size[0]}x{size[1]}{"-ac" if ac else ""}'


@functools.lru_cache(maxsize=None)
def resize_reference(C, hw, size, ac):
    """F.interpolate(mode='bilinear') where in / out is a power of two (or (in - 1) / (out - 1) = 1/2 with
    align_corners): the source coordinates and both weights are multiples of 1/8 per axis, exact in fp32, so y and dx
    are multiples of 1/64.  x in [-2, 2]; gy in {-1, 0, 1}, sparse where many outputs fold onto one input."""
    g = _gen('resize', C, hw, size, ac)
    x = ints((2, C) + tuple(hw), -2, 2, 1.0, g)
    ratio = (size[0] * size[1]) / (hw[0] * hw[1])
    gy = ints((2, C) + tuple(size), -1, 1, 0.9 if ratio <= 4 else 0.1, g)
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, size=tuple(size), mode='bilinear', align_corners=ac)
    y.backward(gy)
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad}


DROPOUT_P = (0.5, 0.75)
DROPOUT_SHAPE = (2, 24, 9, 10)   # 4320 elements


def dropout_operands():
    g = _gen('dropout')
    x = ints(DROPOUT_SHAPE, 1, 3, 1.0, g) * (2 * ints(DROPOUT_SHAPE, 0, 1, 1.0, g) - 1)   # nonzero, both signs
    gy = ints(DROPOUT_SHAPE, 1, 2, 1.0, g) * (2 * ints(DROPOUT_SHAPE, 0, 1, 1.0, g) - 1)
    return x, gy


# ---------------------------------------------------------------------------------------------------------------------
# Tier B: per-element bounds
# ---------------------------------------------------------------------------------------------------------------------
def ulp_store(ref, mode):
    """spacing of the storage dtype at |ref| (fp64 tensor): 2^(e - t) with t = 7 (bf16), 10 (fp16, floor 2^-24: the
    subnormals) or 23 (fp32, floor 2^-149)"""
    t, floor = {'bf16': (7, -133), 'f16': (10, -24), 'f32': (23, -149)}[mode]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -200)))
    return torch.pow(2.0, (e - t).clamp_min(floor))


def q(t, mode):
    """the value the engine sees: t rounded to the storage dtype"""
    return t.to(TORCH_DTYPE[mode]).double()


def assert_bounded(got, ref, M, k, mode, what, fp32=False):
    """|got - ref| <= 1/2 ulp_store(ref) + k 2^-24 M for EVERY element; on a miss the count and the worst few
    (index, got, ref, error, bound) are printed."""
    gd = got.detach().double().cpu()
    assert gd.shape == ref.shape, f'{what}: shape {tuple(gd.shape)} vs {tuple(ref.shape)}'
    bound = 0.5 * ulp_store(ref, 'f32' if fp32 else mode) + k * U24 * M
    err = (gd - ref).abs()
    bad = ~(err <= bound)   # (a NaN fails)
    if bool(bad.any()):
        idx = bad.nonzero()
        worst = (err / bound)[bad].argsort(descending=True)[:8]
        rows = [f'  {tuple(i.tolist())}: got {float(gd[tuple(i.tolist())])!r} ref {float(ref[tuple(i.tolist())])!r} '
                f'err {float(err[tuple(i.tolist())]):.3e} bound {float(bound[tuple(i.tolist())]):.3e}'
                for i in idx[worst]]
        print(f'{what}: {idx.shape[0]} of {gd.numel()} elements outside the bound\n' + '\n'.join(rows))
    assert not bool(bad.any()), f'{what}: outside the per-element bound (details in the captured output)'


BN_EPS = 1e-5


def _bn_random_ref(x, res, gy, gamma, beta, relu, P):
    col = lambda v: v[:, None]  # noqa: E731
    mean = x.sum(1) / P
    var = ((x - col(mean)) ** 2).sum(1) / P
    invstd = 1.0 / (var + BN_EPS).sqrt()
    xh = (x - col(mean)) * col(invstd)
    z = col(gamma) * xh + col(beta) + (res if res is not None else 0.0)
    y = F.relu(z) if relu else z
    dyr = gy * (z > 0) if relu else gy
    mdy, mdyx = dyr.sum(1) / P, (dyr * xh).sum(1) / P
    dx = col(gamma * invstd) * (dyr - col(mdy) - xh * col(mdyx))
    # magnitudes (the M of each element: bn_train_random's docstring)
    ex, ex2 = x.abs().sum(1) / P, (x * x).sum(1) / P
    xh_err = col(invstd) * (x.abs() + col(mean.abs()) + col(ex)) + xh.abs() * col(ex2 * invstd * invstd)
    My = col(gamma.abs()) * xh_err + col(beta.abs()) + (res.abs() if res is not None else 0.0)
    edy, edyx = dyr.abs().sum(1) / P, (dyr * xh).abs().sum(1) / P
    Mdx = col((gamma * invstd).abs()) * (dyr.abs() + col(mdy.abs() + edy)
                                         + (xh.abs() + xh_err) * col(mdyx.abs() + edyx))
    Mdg = (dyr.abs() * (xh.abs() + xh_err)).sum(1)
    Mdb = dyr.abs().sum(1)
    return {'mean': mean, 'var': var, 'invstd': invstd, 'z': z, 'y': y, 'dx': dx, 'dres': dyr,
            'dgamma': (dyr * xh).sum(1), 'dbeta': dyr.sum(1), 'My': My, 'Mdx': Mdx, 'Mdgamma': Mdg, 'Mdbeta': Mdb}


BN_K_FWD, BN_K_BWD, BN_K_PGRAD = 14, 19, 9
BN_MARGIN = 2.0 ** -10   # pre-activations keep |z| >= 2^-10 M >> 14 * 2^-24 M


@functools.lru_cache(maxsize=None)
def bn_train_random(C, nhw, relu, residual, mode):
    """Train-mode BN on randn data (eps 1e-5), the inputs rounded to the storage dtype of `mode`.  With a ReLU the data
    is redrawn (x + 1/4 on the offending elements, re-rounded) until no pre-activation z lies within BN_MARGIN * M of
    0, so that the mask of the reference is the mask of any result inside the bound.

    k (BN_K_FWD, BN_K_BWD, BN_K_PGRAD), counted in csrc/bn.hip:
      forward (bn_apply_kernel): v - mu, * is, fmaf(ga, xh, be), + r = 4; mean and invstd rounded to fp32 = 2; the
      statistics sum each batch of U = 4 pixels in fp32 before the fp64 add (bn_partial_kernel: 4 terms for sum x, 4 for
      sum x^2) = 8.  k = 14 against
      M = |gamma| (invstd (|x| + |mean| + E|x|) + |x_hat| E[x^2] invstd^2) + |beta| + |res|.
      backward (bn_bwd_apply_kernel): gi = ga * is, x_hat (2), xh * mdyx, two subtractions, gi * d = 7; mean, invstd,
      mean(dyr), mean(dyr x_hat) rounded to fp32 = 4; the two backward sums in fp32 batches of 4 = 8; x_hat's own error
      is carried by M.  k = 19 against M = |gamma invstd| (|dyr| + |mean dyr| + E|dyr| + (|x_hat| + x_hat's error scale)
      (|mean dyr x_hat| + E|dyr x_hat|)).
      dgamma / dbeta (fp32 outputs of bn_partial_kernel MODE 1): the fp32 part of the sum is one batch of 4 terms (4:
      the batches are added in fp64), x_hat (2), mean and invstd (2), the fp32 cast of the total (1): k = 9 against
      M = sum |dyr| (|x_hat| + x_hat's error scale) resp. sum |dyr|."""
    g = _gen('bn-random', C, nhw, relu, residual)
    n_, h_, w_ = nhw
    P = n_ * h_ * w_
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = q(rn(C, P) * 1.5 + rn(C, 1), mode)
    res = q(rn(C, P), mode) if residual else None
    gy = q(rn(C, P), mode)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.rand(C, generator=g, dtype=torch.float64) * 0.6 - 0.3).float().double()
    for _ in range(16):
        r = _bn_random_ref(x, res, gy, gamma, beta, relu, P)
        near = (r['z'].abs() < BN_MARGIN * r['My']) if relu else torch.zeros_like(x, dtype=torch.bool)
        if not bool(near.any()):
            break
        x = q(torch.where(near, x + 0.25, x), mode)
    else:
        raise AssertionError('bn_train_random: pre-activations near 0 remain')
    out = {k: (_nchw(v, nhw) if v.dim() == 2 else v) for k, v in r.items()}
    out.update(x=_nchw(x, nhw), gy=_nchw(gy, nhw), res=_nchw(res, nhw) if residual else None, gamma=gamma, beta=beta,
               P=P)
    return out


AVGPOOL3_CASES = ((16, (9, 7)), (24, (13, 11)))
AVG3_K_FWD, AVG3_K_BWD = 10, 8


@functools.lru_cache(maxsize=None)
def avgpool3_random(C, hw, mode):
    """AvgPool2d(3, 2, 1) (count_include_pad: the divisor is 9 except where the window leaves the padded map).

    k, counted in csrc/pool.hip.  avgpool_fwd_kernel: <= 9 taps summed in fp32 (9) and one division (1):
    AVG3_K_FWD = 10 against M = sum |x tap| / div.  avgpool_bwd_kernel: <= 4 windows reach a pixel (kernel 3,
    stride 2), each g / div (4 divisions) and summed (4): AVG3_K_BWD = 8 against M = sum |g| / div."""
    g = _gen('avg3', C, hw)
    x = q(torch.randn((2, C) + tuple(hw), generator=g, dtype=torch.float64), mode)
    xr = x.clone().requires_grad_(True)
    y = F.avg_pool2d(xr, 3, 2, 1)
    gy = q(torch.randn(y.shape, generator=g, dtype=torch.float64), mode)
    y.backward(gy)
    xa = x.abs().requires_grad_(True)
    My = F.avg_pool2d(xa, 3, 2, 1)
    My.backward(gy.abs())
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad, 'My': My.detach(), 'Mdx': xa.grad}


GAP_RANDOM = ((24, 11, 13), (16, 15, 20))   # HW = 143 (one split), 300 (two splits)


def gap_k(HW):
    """gap_partial_kernel + gap_final_kernel: a sum of HW terms in fp32 (HW), inv_hw = (float)(1 / HW) (1) and the
    product s * inv_hw (1): k = HW + 2 against M = sum |x| / HW.  gap_bwd_kernel: inv_hw (1), g * inv_hw (1): k = 2
    against M = |g| / HW."""
    return HW + 2, 2


@functools.lru_cache(maxsize=None)
def gap_random(C, H, W, mode):
    g = _gen('gap-random', C, H, W)
    x = q(torch.randn(2, C, H, W, generator=g, dtype=torch.float64), mode)
    gy = q(torch.randn(2, C, 1, 1, generator=g, dtype=torch.float64), mode)
    xr = x.clone().requires_grad_(True)
    y = F.adaptive_avg_pool2d(xr, 1)
    y.backward(gy)
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad, 'My': F.adaptive_avg_pool2d(x.abs(), 1),
            'Mdx': (gy.abs() / (H * W)).expand_as(x).contiguous()}


RESIZE_RANDOM = ((8, (5, 7), (17, 12), False), (24, (5, 7), (17, 12), True))


def _axis_taps(n_in, n_out, ac):
    """[n_out, n_in] 0/1: the (at most two) inputs an output reads, by PyTorch's source-index rule in fp64"""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for d in range(n_out):
        if ac:
            src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            src = max((d + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        m[d, i0] = 1.0
        m[d, min(i0 + 1, n_in - 1)] = 1.0
    return m


def resize_k(hw, size):
    """src_index: the scale (1), scale * (d + 1/2) (1), - 1/2 (1) carry an ABSOLUTE error of <= 3 * 2^-24 S into both
    weights of an axis (S = the larger input extent bounds the source coordinate), 1 - l1 one more: 3 S + 1 per axis.
    bilinear_fwd_nhwc_kernel: 6 products and 3 sums = 9: k = 9 + 2 (3 S + 1) against M = the sum of the |x| of the 4
    taps (unweighted: the weight errors are absolute).  Backward (rows + cols kernels): one fma per contributing
    output (T = the most outputs that fold onto one input) and one per contributing row (R): k = T + R + 2 (3 S + 1)
    against M = the sum of the |gy| of the contributing outputs (unweighted)."""
    S = max(hw)
    T = (math.ceil(size[0] / hw[0]) * 2 + 1) * (math.ceil(size[1] / hw[1]) * 2 + 1)
    R = math.ceil(size[0] / hw[0]) * 2 + 1
    return 9 + 2 * (3 * S + 1), T + R + 2 * (3 * S + 1)


@functools.lru_cache(maxsize=None)
def resize_random(C, hw, size, ac, mode):
    g = _gen('resize-random', C, hw, size, ac)
    x = q(torch.randn((2, C) + tuple(hw), generator=g, dtype=torch.float64), mode)
    gy = q(torch.randn((2, C) + tuple(size), generator=g, dtype=torch.float64), mode)
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, size=tuple(size), mode='bilinear', align_corners=ac)
    y.backward(gy)
    th, tw = _axis_taps(hw[0], size[0], ac), _axis_taps(hw[1], size[1], ac)
    My = torch.einsum('oh,nchw,pw->ncop', th, x.abs(), tw)
    Mdx = torch.einsum('oh,ncop,pw->nchw', th, gy.abs(), tw)
    return {'x': x, 'gy': gy, 'y': y.detach(), 'dx': xr.grad, 'My': My, 'Mdx': Mdx, 'th': th, 'tw': tw}


ATT_SHAPE = (2, 5, 9, 11)
ATT_K_FWD, ATT_K_G = 8, 6


def att_k_gatt(C):
    return 4 * C + 12


@functools.lru_cache(maxsize=None)
def att_blend_random():
    """lo sigmoid(a) + hi (1 - sigmoid(a)) on fp32 randn data (ops.att_blend is fp32 in every compute mode).

    k, counted in csrc/pool.hip.
    att_blend_fwd_kernel: s = 1 / (1 + expf(-a)): expf within 1 ulp (2), the sum (1), the division (1) = 4 on s, which
    multiplies |lo| + |hi|; then 1 - s, two products, one sum = 4: k = 8 against M = |lo| + |hi|.
    att_blend_bwd_kernel: glo = g s, ghi = g (1 - s): k = 4 + 2 = 6 against M = |g|;
    gatt = (sum_c g lo - g hi) (1 - s) s:
    per channel two products, one difference, one accumulation (4 C), the two closing products (2), s and 1 - s (5 each
    way, counted once on the product: 10): k = 4 C + 12 against M = sum_c |g| (|lo| + |hi|)."""
    g = _gen('att')
    n, c, h, w = ATT_SHAPE
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    lo, hi, att, gy = f(n, c, h, w), f(n, c, h, w), f(n, 1, h, w) * 2, f(n, c, h, w)
    lr, hr, ar = (t.clone().requires_grad_(True) for t in (lo, hi, att))
    s = torch.sigmoid(ar)
    y = lr * s + hr * (1 - s)
    y.backward(gy)
    return {'lo': lo, 'hi': hi, 'att': att, 'gy': gy, 'y': y.detach(), 'dlo': lr.grad, 'dhi': hr.grad,
            'datt': ar.grad, 'My': lo.abs() + hi.abs(), 'Mg': gy.abs(),
            'Matt': (gy.abs() * (lo.abs() + hi.abs())).sum(1, keepdim=True)}
