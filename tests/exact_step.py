"""Operands, host restatements and comparison functions for the plumbing kernels of the training step
(test_step_exact*.py): the layout / dtype converters, the fused clip + SGD step, the squared norm, the teacher EMA, the
loss-scale machinery, axpby / scale / sigmoid (csrc/eltwise.hip) and the pixel mix (ssseg_mix, csrc/cowmix.hip).

Tier A (bit equality).  The kernels' rounding is fixed by their source and build (fmaf, products that feed an fmaf's
addend, one round-to-nearest-even per conversion; one contraction, see sgd_ref), so a restatement in numpy float32
-- with fma32() below for fmaf, which this Python has no builtin for -- must give the device's BITS on random data.
Every restatement cites the kernel lines it follows; test_step_exact_host.py proves each against an independent fp64 /
exact-rational computation and shows that every comparison function here rejects the mutation it exists for.

Tier B (bounded per element).  Where a library function (expf), a division by a sum or a product with a soft mask
enters, EVERY element is held to 1/2 ulp_store(ref) + k 2^-24 M (exact_aux.assert_bounded) with k counted from the
kernel's expression in the docstring of the reference.

All arrays are numpy float32 / CPU torch tensors; nothing here imports ssseg.  The comparison functions take the
device's result as plain host arrays, so the host file can feed them a mutant's output instead.
"""
import functools

import numpy as np
import torch

import exact_aux as A
from exact import TORCH_DTYPE, _gen

U24 = 2.0 ** -24
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# grid-stride caps (csrc/common.h ssseg_grid, 256 threads): elements one sweep covers
SWEEP_DEFAULT = 4096 * 256          # converters, cast, mix, sigmoid, axpby, scale_by (cap 256 * 16 workgroups)
SWEEP_SGD = 2048 * 256              # ssseg_sgd_step, ssseg_scale_f32 (cap 256 * 8)
SWEEP_EMA = 2048 * 256 * 4          # ssseg_ema_update: float4 per thread
SWEEP_RED = 1024 * 256              # ssseg_sqnorm_accum (RED_BLOCKS x RED_THREADS)


# ---------------------------------------------------------------------------------------------------------------------
# 1. fmaf on the host
# ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """round_to_nearest_even_fp32(a * b + c), the product and sum exact: fmaf bit for bit.

    a * b is exact in fp64 (24 + 24 significand bits).  s = fl64(a b + c) and TwoSum gives the exact error e with
    a b + c = s + e, |e| <= 1/2 ulp64(s).  No fp64 number lies strictly between s and s + e, and every fp32 rounding
    boundary (a midpoint of two neighbouring fp32 values: 25 bits) is one, so s and s + e round to the same fp32 value
    UNLESS s sits exactly on a midpoint and e != 0: there the tie rule would decide what e in fact decides, and s is
    moved one fp64 ulp toward the sign of e first."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c)))
    with np.errstate(all='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        f = s.astype(np.float32)
        f64 = f.astype(np.float64)
        other = np.nextafter(f, np.where(s > f64, np.inf, -np.inf).astype(np.float32))   # s lies between f and other
        mid = 0.5 * f64 + 0.5 * other.astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(other) & (f64 != s) & (mid == s) & np.isfinite(e) & (e != 0)
        s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def fma32_naive(a, b, c):
    """the double rounding fma32 exists to avoid (the host file shows it wrong on every constructed tie that breaks to
    the odd neighbour)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def bf16_rne(x):
    """float32 -> the bits of the nearest bfloat16, ties to even (common.h f32_to_bf16), as uint16"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7fff)) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7fc0), out)


def bf16_trunc(x):
    """the mutation: the upper half of the word, no rounding"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same_bits(got, want, what):
    """np.array_equal on the raw bits (so -0.0 != +0.0) over ALL elements; on a miss the count and the first few
    (index, got, want) are printed"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    gb, wb = _bits(got), _bits(want)
    if not np.array_equal(gb, wb):
        bad = np.argwhere(gb != wb)
        rows = [f'  {tuple(i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}' for i in bad[:8]]
        print(f'{what}: {bad.shape[0]} of {got.size} elements differ\n' + '\n'.join(rows))
    assert np.array_equal(gb, wb), f'{what}: differs from the restatement (details in the captured output)'


def same_bits_nan(got, want, what):
    """torch tensors of one dtype: NaN exactly where the reference has NaN (any payload), torch.equal on the raw bits
    everywhere else"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f'{what}: NaN at {int((gn != wn).sum())} wrong places'
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    zero = torch.zeros((), dtype=got.dtype)
    g, w = torch.where(gn, zero, got).contiguous().view(it), torch.where(wn, zero, want).contiguous().view(it)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        rows = [f'  {tuple(i.tolist())}: got {float(got[tuple(i.tolist())])!r} want {float(want[tuple(i.tolist())])!r}'
                for i in bad[:8]]
        print(f'{what}: {bad.shape[0]} of {got.numel()} elements differ\n' + '\n'.join(rows))
    assert torch.equal(g, w), f'{what}: bits differ from the reference (details in the captured output)'


def nondegenerate(t, what):
    """exact_aux.nondegenerate (half nonzero, every channel with distinct values) and every image (dim 0) different
    from every other, so a swapped batch or channel index changes the result.  t: torch tensor with N and C leading."""
    t = torch.as_tensor(t).double()
    t = torch.where(torch.isfinite(t), t, torch.full_like(t, 12345.0))   # (the specials count as values)
    A.nondegenerate(t, what)
    for i in range(t.shape[0]):
        for j in range(i + 1, t.shape[0]):
            assert not torch.equal(t[i], t[j]), f'{what}: images {i} and {j} are equal'
    if t.dim() >= 2:
        for i in range(t.shape[1]):
            for j in range(i + 1, t.shape[1]):
                assert not torch.equal(t[:, i], t[:, j]), f'{what}: channels {i} and {j} are equal'


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. layout and dtype converters (eltwise.hip: the nchw_to_nhwc / nhwc_to_nchw / cast kernels and their entry points)
# ---------------------------------------------------------------------------------------------------------------------
DTYPES = ('f32', 'bf16', 'f16')
DT_CODE = {'f32': 0, 'bf16': 1, 'f16': 2}   # native.F32 / BF16 / F16
# the pairs each entry point dispatches (ssseg_nchw_to_nhwc, ssseg_nhwc_to_nchw, ssseg_cast in eltwise.hip); bf16 <-> f16
# is refused by all three
TO_NHWC_PAIRS = (('f32', 'f32'), ('f32', 'bf16'), ('bf16', 'bf16'), ('bf16', 'f32'), ('f32', 'f16'), ('f16', 'f16'),
                 ('f16', 'f32'))
TO_NCHW_PAIRS = TO_NHWC_PAIRS
CAST_PAIRS = (('f32', 'bf16'), ('bf16', 'f32'), ('f32', 'f32'), ('bf16', 'bf16'), ('f32', 'f16'), ('f16', 'f32'))
REFUSED_PAIRS = (('bf16', 'f16'), ('f16', 'bf16'))
LAYOUT_NHW = (2, 7, 9)
GENERIC_CCP = ((1, 4), (3, 4), (5, 12))                    # Cp % 8 != 0: nchw_to_nhwc_kernel
PIXEL_CCP = ((3, 8), (8, 8), (13, 16), (3, 16))            # Cp % 8 == 0 and an fp32 source: nchw_to_nhwc_pix_kernel
BIG_PIXEL = (1, 3, 1025, 1024, 8)                          # P = 1 049 600 > SWEEP_DEFAULT pixels
BIG_GENERIC = (1, 3, 600, 600, 4)                          # N H W Cp = 1 440 000 > SWEEP_DEFAULT elements
BIG_NCHW = (1, 3, 600, 600, 4)                             # N H W C = 1 080 000 > SWEEP_DEFAULT elements
HEAD_VIEW = (2, 8)                                         # the heads' 2-channel view of an 8-channel buffer
CAST_N = (1, 257, 2 ** 20 + 5)

SPECIALS = {
    '+0': 0.0, '-0': -0.0, '+inf': float('inf'), '-inf': float('-inf'), 'nan': float('nan'),
    'FLT_MAX': FLT_MAX, '-FLT_MAX': -FLT_MAX,
    # exact ties of the bf16 rounding (8 significand bits), both parities: to 1 (even, down) and to 1 + 2^-6 (even, up)
    'bf16 tie down': 1 + 2.0 ** -8, 'bf16 tie up': 1 + 3 * 2.0 ** -8, '-bf16 tie up': -(1 + 3 * 2.0 ** -8),
    # exact ties of the fp16 rounding (11 bits)
    'f16 tie down': 1 + 2.0 ** -11, 'f16 tie up': 1 + 3 * 2.0 ** -11, '-f16 tie down': -(1 + 2.0 ** -11),
    # fp16 overflow: 65520 is the midpoint of 65504 and 2^16 and rounds to inf; the fp32 value below it stays finite
    'f16 overflow': 65520.0, 'f16 below overflow': float(np.nextafter(np.float32(65520.0), np.float32(0.0))),
    '-f16 overflow': -65520.0,
    # fp16's subnormal range (multiples of 2^-24): representable, a tie to 0, a tie up, an inexact one, the smallest
    # normal, and a value under half the smallest subnormal
    'f16 sub': 3 * 2.0 ** -24, 'f16 sub tie0': 2.0 ** -25, 'f16 sub tie up': 3 * 2.0 ** -25,
    'f16 sub inexact': float(np.float32(1e-7)),
    'f16 min normal': 2.0 ** -14, 'f16 sub under': -(2.0 ** -26),
    # fp32 subnormals: bf16 keeps 2^-130, rounds 3 * 2^-135 (a tie of its subnormal grid 2^-133) and loses 2^-149
    'f32 sub': 2.0 ** -130, 'f32 sub tie': -3 * 2.0 ** -135, 'f32 min sub': 2.0 ** -149,
}
SPECIAL_VALUES = torch.tensor(list(SPECIALS.values()), dtype=torch.float64).float()


def specials_present(x, dt_in):
    """every special (as dt_in holds it) occurs in x"""
    want = SPECIAL_VALUES.to(TORCH_DTYPE[dt_in])
    it = {2: torch.int16, 4: torch.int32}[want.element_size()]
    have = set(x.contiguous().view(it).flatten().tolist())
    return all((v in have) for v in want.view(it).tolist())


@functools.lru_cache(maxsize=None)
def values(shape, dt_in, key='v', lanes=None):
    """fp32 standard normals, each times one of {1, 2^-10, 2^10}, with every SPECIALS value planted at a place of its
    own (where the tensor has room; a shorter one takes them in order), rounded to dt_in by torch's CPU cast.
    lanes: the specials go only where the index of the last dimension is < lanes (the lanes c < C an NHWC reader with
    ldc > C reads)."""
    g = _gen('step-values', tuple(shape), key, lanes)
    n = int(np.prod(shape))
    x = _randn(g, n) * torch.tensor([1.0, 2.0 ** -10, 2.0 ** 10])[torch.randint(0, 3, (n,), generator=g)]
    places = torch.arange(n) if lanes is None else torch.arange(n).view(*shape)[..., :lanes].flatten()
    k = min(places.numel(), SPECIAL_VALUES.numel())
    where = places[torch.randperm(places.numel(), generator=g)[:k]]
    x[where] = SPECIAL_VALUES[:k]
    return x.view(*shape).to(TORCH_DTYPE[dt_in])


def to_nhwc_ref(x, Cp, dt_out):
    """[N, C, H, W] -> [N, H, W, Cp]: permute, one cast, +0.0 in the lanes c >= C (nchw_to_nhwc_kernel and
    nchw_to_nhwc_pix_kernel, eltwise.hip)"""
    n, c, h, w = x.shape
    y = torch.zeros(n, h, w, Cp, dtype=TORCH_DTYPE[dt_out])
    y[..., :c] = x.permute(0, 2, 3, 1).float().to(TORCH_DTYPE[dt_out])
    return y


def to_nchw_ref(x, C, dt_out):
    """[N, H, W, ldc] -> [N, C, H, W] of its first C lanes (nhwc_to_nchw_kernel, eltwise.hip)"""
    return x[..., :C].permute(0, 3, 1, 2).float().to(TORCH_DTYPE[dt_out]).contiguous()


def cast_ref(x, dt_out):
    return x.float().to(TORCH_DTYPE[dt_out])


def to_nhwc_mutant(x, Cp, dt_out, kind, fill):
    """what a wrong converter would leave in a destination prefilled with `fill`: 'pad' leaves the lanes c >= C
    unwritten, 'stride' reads channel c at stride Cp instead of HW"""
    n, c, h, w = x.shape
    y = to_nhwc_ref(x, Cp, dt_out)
    if kind == 'pad':
        y[..., c:] = fill
    elif kind == 'stride':
        flat = x.float().flatten()
        ni, pi, ci = torch.meshgrid(torch.arange(n), torch.arange(h * w), torch.arange(c), indexing='ij')
        src = (ni * c * h * w + ci * Cp + pi) % flat.numel()
        y[..., :c] = flat[src].view(n, h, w, c).to(TORCH_DTYPE[dt_out])
    else:
        raise ValueError(kind)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# 3. clip + SGD (sgd_kernel, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
SGD_LR, SGD_N, SGD_S = 0.05, 1027, 1024.0
SGD_MOM, SGD_WD, SGD_CLIP, SGD_AMP = (0.0, 0.9), (0.0, 5e-4), ('off', 'above', 'below'), (False, True)
SGD_SIZES = (1, 255, 257, SWEEP_SGD + 3)
SGD_COEF_K = 6


def sgd_ref(p, g, buf, coef, lr, mom, wd, first, want_shadow, contract=True):
    """sgd_kernel's loop body (eltwise.hip) given the scalar coefficient it applied:
        gi = g * coef                       (written back to g)
        d  = fma(p, wd, gi) if wd != 0 else gi
        b  = d if first else fma(buf, mom, d)   (only when mom != 0, else b = d and buf is not touched)
        p' = fma(b, -lr, p);  shadow = bf16_rne(p')
    The source spells the momentum update __fadd_rn(__fmul_rn(buf, mom), d), but HIP defines both as the plain
    operators, and eltwise.hip is compiled with the default -ffp-contract=fast: the pair compiles to ONE fma (the ISA of
    sgd_kernel has a v_fmac_f32 there and no separate product), one rounding where torch's buf.mul_(mom).add_(d) has
    two.  The restatement follows the device; contract=False is the two-rounding form, which the host
    file shows sgd_check tells apart.  g * coef feeds an fmaf's addend or has two uses, and is never fused.
    Returns (p', g', buf', shadow bits or None)."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    coef, lr, mom, wd = F32(coef), F32(lr), F32(mom), F32(wd)
    gi = g * coef
    d = fma32(p, wd, gi) if wd != 0 else gi
    if mom != 0:
        if first:
            b = d
        else:
            b = fma32(np.asarray(buf, F32), mom, d) if contract else (np.asarray(buf, F32) * mom) + d
        nbuf = b
    else:
        b, nbuf = d, buf
    np_ = fma32(b, -lr, p)
    return np_, gi, nbuf, (bf16_rne(np_) if want_shadow else None)


def clip_coef_ref(sq, max_norm, unscale):
    """the coefficient of sgd_kernel (eltwise.hip, the lines before its loop) in fp64: unscale * min(max_norm /
    (sqrt(sq) unscale + 1e-6), 1), unscale alone without a clip"""
    sq, max_norm, unscale = float(sq), float(max_norm), float(unscale)
    if max_norm <= 0:
        return unscale
    return unscale * min(max_norm / (np.sqrt(sq) * unscale + 1e-6), 1.0)


def clip_coef_f32(sq32, max_norm, unscale, mutate=None):
    """the same lines in float32, as the device evaluates them (a model of the device for the host file; the GPU
    comparison never uses it).  mutate: 'unscale-late' clips the scaled norm and unscales after, 'no-eps'."""
    sq32, max_norm, coef = F32(sq32), F32(max_norm), F32(unscale)
    if max_norm > 0:
        eps = F32(0.0) if mutate == 'no-eps' else F32(1e-6)
        if mutate == 'unscale-late':
            return F32(F32(min(max_norm / (np.sqrt(sq32) + eps), F32(1.0))) * coef)
        total = np.sqrt(sq32) * coef
        coef = coef * F32(min(max_norm / (total + eps), F32(1.0)))
    return F32(coef)


@functools.lru_cache(maxsize=None)
def sgd_operands(n, amp):
    """p, buf: standard normals (buf nonzero: a first step must ignore it); g: normals x 3 (x S under amp) with element
    0 planted as exactly 1 (S under amp), so that g'[0] / S IS the coefficient the device applied.  sq: the fp64
    squared norm of g as the device sees it."""
    g_ = _gen('sgd', n, amp)
    S = SGD_S if amp else 1.0
    p, buf = _randn(g_, n).numpy(), _randn(g_, n).numpy()
    buf[buf == 0] = 1.0
    g = (_randn(g_, n) * 3).numpy() * F32(S)
    g[0] = S
    sq = float(np.sum(g.astype(np.float64) ** 2))
    return {'p': p, 'g': g, 'buf': buf, 'S': S, 'sq': sq, 'norm': float(np.sqrt(sq)) / S}


def sgd_max_norm(op, clip):
    """the clip threshold as the kernel receives it (a float32): off, 2 x the unscaled norm, 1/4 of it"""
    return float(F32({'off': 0.0, 'above': 2.0, 'below': 0.25}[clip] * op['norm']))


def sgd_check(got, op, mom, wd, max_norm, amp, first, what):
    """got: the device's p, g, buf (None when mom == 0), shadow bits (None when not asked for).
    (a) The coefficient the device applied, c = g'[0] / S (exact: S is a power of two and g[0] = S), is held to
    clip_coef_ref of the fp64 squared norm within SGD_COEF_K 2^-24 relative.  Counted from sgd_kernel's clip block: the
    fp32 rounding of the accumulated norm (1/2 after the root; counted 1, which also covers the summation order of the
    fp64 accumulation), sqrtf, * coef, + 1e-6f, the division, the final * coef: k = 6 (a contraction removes one).
    (b) With c, every element of p', g', buf' and the shadow equals sgd_ref bit for bit, the planted one included."""
    S = op['S']
    c = F32(got['g'][0]) / F32(S)
    want = clip_coef_ref(op['sq'], max_norm, 1.0 / S if amp else 1.0)
    err = abs(float(c) - want)
    print(f'{what}: coefficient {float(c)!r} reference {want!r} error {err / want / U24:.3f} x 2^-24')
    assert err <= SGD_COEF_K * U24 * abs(want), f'{what}: coefficient {float(c)!r} vs {want!r}'
    rp, rg, rb, rs = sgd_ref(op['p'], op['g'], op['buf'], c, SGD_LR, mom, wd, first, got.get('shadow') is not None)
    same_bits(got['p'], rp, f'{what}: p')
    same_bits(got['g'], rg, f'{what}: g')
    if mom != 0:
        same_bits(got['buf'], rb, f'{what}: buf')
    if rs is not None:
        same_bits(got['shadow'], rs, f'{what}: shadow')


def sgd_device_model(op, mom, wd, max_norm, amp, first, shadow, mutate=None):
    """What a device that follows sgd_kernel returns for `op` (the norm rounded once to fp32, clip_coef_f32, sgd_ref),
    or one that carries a named fault:
      'wd-after-momentum'  b = buf mom + gi, then the decay is added to the update: p' = p - lr (b + wd p)
      'first-ignored'      the momentum buffer is blended on the first step too
      'two-roundings'      buf * mom rounded before d is added (what the source's intrinsics suggest; see sgd_ref)
      'unscale-late', 'no-eps'  (clip_coef_f32)
      'shadow-trunc'       the shadow is truncated, not rounded
      'g-not-written'      the scaled gradient is not written back"""
    coef = clip_coef_f32(F32(op['sq']), max_norm, 1.0 / op['S'] if amp else 1.0, mutate)
    p, g, buf = op['p'], op['g'], op['buf']
    if mutate == 'wd-after-momentum':
        gi = g * coef
        b = (gi if first else fma32(buf, F32(mom), gi)) if mom != 0 else gi
        rp = fma32(fma32(p, F32(wd), b), -F32(SGD_LR), p)
        rb, rg, rs = (b if mom != 0 else buf), gi, bf16_rne(rp) if shadow else None
    else:
        rp, rg, rb, rs = sgd_ref(p, g, buf, coef, SGD_LR, mom, wd, first and mutate != 'first-ignored', shadow,
                                 contract=mutate != 'two-roundings')
    if mutate == 'shadow-trunc':
        rs = bf16_trunc(rp)
    if mutate == 'g-not-written':
        rg = g.copy()
    return {'p': rp, 'g': rg, 'buf': rb if mom != 0 else None, 'shadow': rs}


# ---------------------------------------------------------------------------------------------------------------------
# 4. squared norm (sq_partial_kernel, sq_final_kernel, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
SQ_SIZES = (1, 63, 65, 257, SWEEP_RED + 7)


@functools.lru_cache(maxsize=None)
def sq_ints(n, which):
    """integer-valued fp32 in [-8, 8]: every square, every partial sum in any order and both totals are integers
    below 2^24 (the host file asserts it)"""
    g = _gen('sq-ints', n, which)
    x = torch.randint(-8, 9, (n,), generator=g).float().numpy()
    if n == 1:
        x[0] = 3.0 + which
    return x


@functools.lru_cache(maxsize=None)
def sq_normals(n):
    return _randn(_gen('sq-normals', n), n).numpy()


def sq_check_bounded(out, x, what):
    """|out - ref| <= 1/2 ulp32(ref) + n 2^-53 ref with ref the fp64 sum of the exact squares: the kernel squares and
    accumulates in fp64 (each v * v exact, the n additions of any order within n 2^-53 of the sum of these positive
    terms) and rounds once to fp32"""
    ref = float(np.sum(x.astype(np.float64) ** 2))
    bound = 0.5 * float(A.ulp_store(torch.tensor(ref, dtype=torch.float64), 'f32')) + x.size * 2.0 ** -53 * ref
    err = abs(float(out) - ref)
    print(f'{what}: out {float(out)!r} ref {ref!r} err {err:.3e} bound {bound:.3e}')
    assert err <= bound, f'{what}: {float(out)!r} vs {ref!r}'


# ---------------------------------------------------------------------------------------------------------------------
# 5. EMA (ema_kernel, ssseg_ema_update, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
# the last: ssseg_grid(n / 4 + 1, 256, 2048) caps at 2048 * 256 threads, so the float4 loop takes a second iteration
# only when n / 4 > 2048 * 256: one float4 of a second sweep and a 3-element tail (SWEEP_EMA + 3 is still one sweep)
EMA_SIZES = (1, 3, 4, 5, 1023, SWEEP_EMA + 4 + 3)
EMA_ALPHAS = (0.99, 0.999)


def ema_ref(e, p, alpha, mutate=None):
    """a = float32(alpha), beta = float32(1.0 - alpha) with the subtraction in fp64 (ssseg_ema_update, eltwise.hip);
    e' = fma(p, beta, e * a) (:188).  mutate='beta32': beta = float32(1) - float32(alpha)."""
    a = F32(alpha)
    beta = F32(1.0) - a if mutate == 'beta32' else F32(1.0 - float(alpha))
    return fma32(p, beta, np.asarray(e, F32) * a)


@functools.lru_cache(maxsize=None)
def ema_operands(n):
    g = _gen('ema', n)
    return _randn(g, n).numpy(), _randn(g, n).numpy()


def ema_check(got, e, p, alpha, what):
    same_bits(got, ema_ref(e, p, alpha), what)


# ---------------------------------------------------------------------------------------------------------------------
# 6. loss scale (amp_update_kernel, scale_by_kernel, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
AMP_INIT, AMP_BACKOFF, AMP_INTERVAL = 8.0, 0.5, 3
AMP_GROWTHS = (2.0, 1.5)
INF, NAN = float('inf'), float('nan')
# finite x 3 (grows at the third), inf, nan, finite x 2, inf, then overflows to the floor of 1.0 and past it, then
# three finite steps that grow from the floor
AMP_SCRIPT = (1.0, 4.0, 9.0, INF, NAN, 2.0, 3.0, INF, INF, INF, INF, 1.0, 1.0, 1.0)
# (scale, growth tracker, found_inf) after each scripted step, written out by hand from the rule
AMP_EXPECT = {
    2.0: ((8, 1, 0), (8, 2, 0), (16, 0, 0), (8, 0, 1), (4, 0, 1), (4, 1, 0), (4, 2, 0), (2, 0, 1), (1, 0, 1),
          (1, 0, 1), (1, 0, 1), (1, 1, 0), (1, 2, 0), (2, 0, 0)),
    1.5: ((8, 1, 0), (8, 2, 0), (12, 0, 0), (6, 0, 1), (3, 0, 1), (3, 1, 0), (3, 2, 0), (1.5, 0, 1), (1, 0, 1),
          (1, 0, 1), (1, 0, 1), (1, 1, 0), (1, 2, 0), (1.5, 0, 0)),
}
SCALE_N = (1, 257, 2 ** 20 + 5)


def amp_initial(scale=AMP_INIT):
    return np.array([scale, 0.0, 0.0, 1.0 / scale], dtype=np.float32)


def amp_ref(state, sq, growth, backoff, interval):
    """amp_update_kernel (eltwise.hip) in float32: state = [scale, growth tracker, found_inf, 1 / scale]"""
    st = np.array(state, dtype=np.float32)
    sc, growth, backoff = st[0], F32(growth), F32(backoff)
    if not np.isfinite(F32(sq)):
        sc = max(F32(sc * backoff), F32(1.0))
        st[1], st[2] = 0.0, 1.0
    else:
        st[2] = 0.0
        st[1] = st[1] + F32(1.0)
        if st[1] >= F32(interval):
            sc = F32(sc * growth)
            st[1] = 0.0
    st[0] = sc
    st[3] = F32(1.0) / F32(sc)
    return st


def amp_script(growth):
    """the state after every step of AMP_SCRIPT"""
    st, out = amp_initial(), []
    for sq in AMP_SCRIPT:
        st = amp_ref(st, sq, growth, AMP_BACKOFF, AMP_INTERVAL)
        out.append(st.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 7. axpby, scale (axpby_kernel, scale_kernel, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
AXPBY_N = (1, 257, 2 ** 20 + 5)
AXPBY_AB = ((1.0, 1.0), (0.5, 10.0), (-0.3, 0.7))
AXPBY_A = (1.0, 0.1)
SCALE_F32_N = (1, SWEEP_SGD + 5)


def axpby_ref(x, a, y=None, b=0.0):
    """out = fma(a, x, b * y), or a * x without y (axpby_kernel, eltwise.hip)"""
    x = np.asarray(x, F32)
    if y is None:
        return x * F32(a)
    return fma32(F32(a), x, np.asarray(y, F32) * F32(b))


def scale_ref(x, a):
    """x * a in float32 (scale_kernel :304, scale_by_kernel :291)"""
    return np.asarray(x, F32) * F32(a)


@functools.lru_cache(maxsize=None)
def vec(n, key):
    return _randn(_gen('step-vec', n, key), n).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 8. sigmoid (sigmoidf_ref, sigmoid_fwd_kernel, sigmoid_bwd_kernel, eltwise.hip)
# ---------------------------------------------------------------------------------------------------------------------
SIGMOID_N = (4099, SWEEP_DEFAULT + 5)
SIGMOID_SPECIALS = (0.0, 20.0, -20.0, 90.0, -90.0, INF, -INF)
SIGMOID_K_FWD, SIGMOID_K_BWD = 4, 3


@functools.lru_cache(maxsize=None)
def sigmoid_operands(n):
    """x: standard normals x 4 with SIGMOID_SPECIALS planted first; gy: standard normals"""
    g = _gen('sigmoid', n)
    x, gy = (_randn(g, n) * 4).numpy(), _randn(g, n).numpy()
    x[:len(SIGMOID_SPECIALS)] = SIGMOID_SPECIALS
    return x, gy


def sigmoid_overflows(x):
    """the inputs whose expf(-x) overflows fp32 (x < -88.72...) without x being -inf: there 1 / (1 + inf) is exactly
    +0 on the device while the true value is a positive number under 2^-128"""
    with np.errstate(over='ignore'):
        return np.isfinite(x) & (np.exp(-x.astype(np.float64)) >= 2.0 ** 128)


def sigmoid_check_fwd(got, x, what):
    """y = 1 / (1 + expf(-x)) (sigmoidf_ref, eltwise.hip).  k = SIGMOID_K_FWD = 4, the count att_blend_random
    documents for the same expression: expf within 1 ulp (2), the sum (1), the division (1); a relative error of e =
    exp(-x) reaches y scaled by e / (1 + e) < 1, so M = |ref|.  Exactly 0, 1 and 1/2 at -inf, +inf and 0.  Where
    expf(-x) overflows (sigmoid_overflows) the documented result is exactly +0.0."""
    x64 = x.astype(np.float64)
    with np.errstate(over='ignore'):
        ref = 1.0 / (1.0 + np.exp(-x64))
    over = sigmoid_overflows(x)
    same_bits(got[over], np.zeros(int(over.sum()), F32), f'{what}: expf overflow')
    for v, r in ((-INF, 0.0), (INF, 1.0), (0.0, 0.5)):
        m = x == v
        same_bits(got[m], np.full(int(m.sum()), r, F32), f'{what}: sigmoid({v})')
    keep = torch.from_numpy(~over)
    rt = torch.from_numpy(ref)
    A.assert_bounded(torch.from_numpy(got)[keep], rt[keep], rt[keep].abs(), SIGMOID_K_FWD, 'f32', what)


def sigmoid_check_bwd(got, v, gy, what):
    """gx = gy * (v * (1 - v)) (sigmoid_bwd_kernel, eltwise.hip) with v the stored forward output:
    1 - v, v * (...), gy * (...): k = SIGMOID_K_BWD = 3 against M = |gy v (1 - v)| in fp64 on the stored v"""
    v64, g64 = torch.from_numpy(v.astype(np.float64)), torch.from_numpy(gy.astype(np.float64))
    ref = g64 * (v64 * (1.0 - v64))
    A.assert_bounded(torch.from_numpy(got), ref, ref.abs(), SIGMOID_K_BWD, 'f32', what)


# ---------------------------------------------------------------------------------------------------------------------
# 9. mix (mix_kernel, cowmix.hip)
# ---------------------------------------------------------------------------------------------------------------------
MIX_SHAPES = ((2, 3, 5, 7), (2, 3, 419, 419))   # 210 elements; 1 053 366 > SWEEP_DEFAULT
MIX_K = 3


@functools.lru_cache(maxsize=None)
def mix_operands(shape, mode, soft):
    """a, b [B, C, H, W] standard normals rounded to the storage dtype (different in every channel and image);
    mask [B, 1, H, W] fp32, binary and different per image, or soft in (0, 1)"""
    g = _gen('mix', tuple(shape), soft)
    B, C, H, W = shape
    a, b = (_randn(g, *shape).to(TORCH_DTYPE[mode]) for _ in range(2))
    u = torch.rand(B, 1, H, W, generator=g, dtype=torch.float32)
    m = u.clamp(2.0 ** -20, 1 - 2.0 ** -20) if soft else (u > 0.5).float()
    return a, b, m


def mix_binary_ref(a, b, m):
    """a binary mask selects: a * 1 + b * 0 and a * 0 + b * 1 are exact (finite data)"""
    return torch.where(m.bool(), a, b)


def mix_wrong_mask(a, b, m):
    """the mutation: mask[b] read as mask[b * C + c] (wrapped into the mask)"""
    B, C = a.shape[:2]
    idx = (torch.arange(B)[:, None] * C + torch.arange(C)[None, :]) % B
    return torch.where(m[:, 0][idx].bool(), a, b)


def mix_check_binary(got, a, b, m, what):
    same_bits_nan(got, mix_binary_ref(a, b, m), what)


def mix_check_soft(got, a, b, m, mode, what):
    """v = a m + b (1 - m) (mix_kernel, cowmix.hip) in fp32 from the stored a, b, rounded once to the storage
    dtype: the roundings are 1 - m, two products and the sum; the error of 1 - m reaches the element times |b|, each
    product's its own term, the sum's at most |a| m + |b| (1 - m): together under MIX_K = 3 times 2^-24 (|a| + |b|)
    (a contraction removes one, never adds)."""
    a64, b64, m64 = a.double(), b.double(), m.double()
    ref = a64 * m64 + b64 * (1.0 - m64)
    A.assert_bounded(got, ref, a64.abs() + b64.abs(), MIX_K, mode, what)
