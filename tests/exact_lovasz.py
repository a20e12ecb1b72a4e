"""Designed-rank inputs of the Lovász losses and their expectations (no GPU): the builders of
tests/test_lovasz_geometry.py (device) and tests/test_lovasz_geometry_host.py (the proof of the designs on the CPU).

Design.  Per segment (group, class channel) of n valid pixels a permutation `rank` is drawn, and the error of pixel p
is  e = (n - rank[p]) * floor(2^24 / n) * 2^-24 : distinct multiples of 2^-24 in (0, 1], so the sorted position of
every pixel is known without sorting.  'probas' inputs are x = e on background and 1 - e on foreground: both exact in
fp32, and |fg - x| == e bit for bit.  The hinge uses errors ((n - rank) - n // 4) * floor(2^22 / n) * 2^-22 on both
sides of 0 (one of them exactly 0) and x = (1 - err) * (2 fg - 1).  Every class channel has its own permutation; the
foreground of channel c is [label == c].

The expectation follows lovasz_ref.lovasz step by step (fp32 Jaccard steps, fp64 dot rounded to fp32, fp32 means in
index order) with the sort replaced by the designed ranks; the host file shows that it equals lovasz_ref.lovasz bit
for bit.  The gradient is returned in fp64, before the upstream factor."""
import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

import lovasz_ref
from oracle.losses_ref import lovasz_grad

F32, F64 = np.float32, np.float64

# launch thresholds of csrc/lovasz.hip (line numbers of that file) and csrc/common.h, by the names used there
TILE = 2048               # :28 `constexpr int TILE = LT * ITEMS`: one block of hist / scatter / grad
SCAN_ROUND = 64           # :100 seg_rowscan_kernel `t0 += 64`; :696 gen_segsum, :270 lovasz_final_kernel `t += 64`
GRID_SPAN = 256 * 16 * 256     # common.h ssseg_grid_cap(): 256 * 16 blocks, of 256 threads: prep / bwd / softmax-bwd
COUNT_SPAN = 64 * 256     # :871 gen_core: lovasz_gen_count_kernel on at most 64 blocks of 256 per group
COUNT_CAP = 64 * 16 * 256      # :870 cblocks = ceil(L / (256 * 16)) capped at 64: more than 16 rounds per block above
FINAL_GROUPS = 256        # :709 lovasz_gen_final_kernel `g += 256`
BIN_FINAL_IMAGES = 16     # :268 lovasz_final_kernel `b += nw`, nw = FIN_T / 64
CHUNK_KEYS = 1 << 22      # :513 GEN_CHUNK_KEYS
CHUNK_CLASSES = 8         # :512 GEN_CHUNK_CLASSES
MAX_L = 1 << 24           # :846 gen_setup: L > 2^24 -> SSSEG_EINVAL
MAX_S = 65535             # :846 gen_setup: G * nsel > 65535 -> SSSEG_EINVAL

# fp32 roundings between the fp32 Jaccard step g (bitwise the reference's) and the stored gradient, counted in
# lovasz_gen_bwd_kernel / lovasz_gen_final_kernel:  w = 1.f / ((float)nc * (float)G)  [1: the division; nc * G < 2^24
# is exact]   wscale * go  [2]   gpix * (...)  [3].   The sign, and the doubling where a channel is selected twice, are
# exact.  lovasz_bwd_kernel (binary): valid / denom [1], (-sg * gpix) * wscale [2], * go [3].
K_ROUND = 3
ULP = 2.0 ** -24
UPSTREAM = F32(0.5)       # a power of two: rounding [2] is exact


def tiles(n):
    return -(-n // TILE)


def chunk_classes(N, K):
    """gen_chunk: classes sorted at a time"""
    return int(min(K, CHUNK_CLASSES, max(1, CHUNK_KEYS // N)))


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


@dataclass(frozen=True)
class Spec:
    name: str
    B: int
    C: int
    HW: int
    mode: str = 'probas'
    classes: Union[str, Tuple[int, ...]] = 'all'
    per_image: bool = False
    ignore: Optional[int] = None
    void: Optional[str] = None          # pattern of void pixels (see _void_mask)
    absent: Optional[Tuple[int, int]] = None   # (image, class): the image's pixels of the class get the label C
    nofg: Optional[int] = None          # binary entry: this image has no foreground

    @property
    def classes_arg(self):
        return self.classes if isinstance(self.classes, str) else list(self.classes)

    @property
    def G(self):
        return self.B if self.per_image else 1

    @property
    def L(self):
        return self.HW if self.per_image else self.B * self.HW

    @property
    def K(self):
        return self.C if isinstance(self.classes, str) else len(self.classes)


def _void_mask(spec):
    """void pixels of the one 264,193-pixel image: `nvalid` stay valid"""
    m = np.zeros(spec.B * spec.HW, bool)
    if spec.void is None:
        return m
    kind, nvalid = spec.void.split(':')
    nvoid = spec.HW - int(nvalid)
    if kind == 'last':            # one valid pixel, the last one
        m[:nvoid] = True
    elif kind == 'runs':          # a run over many whole tiles and a run of 777 across a tile edge
        m[2 * TILE:2 * TILE + nvoid - 777] = True
        m[100 * TILE - 300:100 * TILE + 477] = True
    else:
        raise KeyError(spec.void)
    assert int(m.sum()) == nvoid
    return m


@dataclass(frozen=True)
class Design:
    x: np.ndarray          # [B, C, 1, HW] f32
    lab: np.ndarray        # [B, 1, HW] int64
    rank: np.ndarray       # [C, B*HW] int32: sorted position of the pixel in its segment, -1 for void pixels


def group_pixels(spec):
    N = spec.B * spec.HW
    return [np.arange(b * spec.HW, (b + 1) * spec.HW) for b in range(spec.B)] if spec.per_image else [np.arange(N)]


def design_errors(spec, n, pos):
    """the designed error at sorted position pos of a segment of n valid pixels, exact in fp64 and in fp32"""
    pos = np.asarray(pos, np.int64)
    if spec.mode == 'hinge':
        q = (1 << 22) // n
        assert q >= 1
        return ((n - pos) - n // 4) * q * 2.0 ** -22
    q = (1 << 24) // n
    assert q >= 1
    return (n - pos) * q * 2.0 ** -24


@functools.lru_cache(maxsize=2)
def build(spec):
    B, C, HW = spec.B, spec.C, spec.HW
    N = B * HW
    rng = np.random.default_rng(zlib.crc32(spec.name.encode()))
    if C == 1 or spec.mode == 'hinge':
        lab = (rng.random(N) < 0.4).astype(np.int64)
    elif C == 2:
        lab = (rng.random(N) < 0.4).astype(np.int64)
    else:
        lab = rng.integers(0, C, N)
    if spec.absent is not None:
        b, c = spec.absent
        seg = lab[b * HW:(b + 1) * HW]
        seg[seg == c] = C      # a label outside the classes: background for all of them
    if spec.nofg is not None:
        for b in range(B):      # exactly one image without foreground
            if not lab[b * HW:(b + 1) * HW].any():
                lab[b * HW + b % HW] = 1
        lab[spec.nofg * HW:(spec.nofg + 1) * HW] = 0
    lab[_void_mask(spec)] = 255
    x = np.full((C, N), 0.5, F32)
    rank = np.full((C, N), -1, np.int32)
    for idx in group_pixels(spec):
        valid = idx[lab[idx] != spec.ignore] if spec.ignore is not None else idx
        n = valid.size
        if n == 0:
            continue
        for ch in range(C):
            r = rng.permutation(n)
            fg = lab[valid] == (1 if C == 1 else ch)
            e = design_errors(spec, n, r)
            if spec.mode == 'hinge':
                x[ch, valid] = (1.0 - e) * np.where(fg, 1.0, -1.0)
            else:
                x[ch, valid] = np.where(fg, 1.0 - e, e)
            rank[ch, valid] = r
    x = np.ascontiguousarray(x.reshape(C, B, HW).transpose(1, 0, 2)).reshape(B, C, 1, HW)
    lab = lab.reshape(B, 1, HW)
    for a in (x, lab, rank):
        a.setflags(write=False)
    return Design(x, lab, rank)


@dataclass(frozen=True)
class Expected:
    loss: np.float32
    grad: np.ndarray       # [B, C, 1, HW] f64, before the upstream factor
    exact: bool            # classes counted * G is a power of two in every group: the device gradient is exact
    diversity: float       # share of adjacent sorted positions (all segments) whose weights differ bitwise
    nseg: int
    grad32: np.ndarray     # the gradient under UPSTREAM in fp32, operation by operation as the kernels compute it


def _diversity_counts(jg):
    b = jg.view(np.uint32)
    return int((b[1:] != b[:-1]).sum()), b.size - 1


@functools.lru_cache(maxsize=2)
def expected(spec):
    """lovasz_ref.lovasz with the stable argsort replaced by the designed ranks"""
    d = build(spec)
    B, C, HW = spec.B, spec.C, spec.HW
    lab = d.lab.reshape(-1)
    ids, present = lovasz_ref.class_ids(spec.classes_arg, C)
    K, G = len(ids), spec.G
    seg_loss = np.zeros((G, K), F32)
    counted = np.zeros((G, K), bool)
    weights = {}
    differ = pairs = 0
    for g, idx in enumerate(group_pixels(spec)):
        valid = idx[lab[idx] != spec.ignore] if spec.ignore is not None else idx
        n = valid.size
        for k, c in enumerate(ids):
            ch = 0 if C == 1 else c
            fg = (lab[valid] == c).astype(F32)
            counted[g, k] = not (present and fg.sum() == 0)
            if n == 0:
                continue
            r = d.rank[ch, valid]
            inv = np.empty(n, np.int64)
            inv[r] = np.arange(n)
            jg = lovasz_grad(fg[inv])
            if counted[g, k]:
                a, b = _diversity_counts(jg)
                differ, pairs = differ + a, pairs + b
            err = design_errors(spec, n, np.arange(n))
            es = np.maximum(err, 0) if spec.mode == 'hinge' else err
            seg_loss[g, k] = F32(np.dot(es, jg.astype(F64)))
            if spec.mode == 'hinge':
                de = np.where(design_errors(spec, n, r) > 0, -(2.0 * fg - 1.0), 0.0)
            else:
                de = np.where(fg > 0, -1.0, 1.0)
            weights[g, k] = (ch, valid, jg[r], de)
    total = F32(0.0)
    dp = np.zeros((C, B * HW), F64)
    dp32 = np.zeros((C, B * HW), F32)
    exact = True
    for g in range(G):
        acc, n = F32(0.0), 0
        for k in range(K):
            if counted[g, k]:
                acc = F32(acc + seg_loss[g, k])
                n += 1
        total = F32(total + (acc / F32(n) if n > 1 else acc))
        exact = exact and (n == 0 or is_pow2(n * G))
        for k in range(K):
            if counted[g, k] and (g, k) in weights:
                ch, valid, w, de = weights[g, k]
                dp[ch, valid] += w.astype(F64) * de / (n * G)
                scale = F32(F32(F32(1.0) / (F32(n) * F32(G))) * UPSTREAM)     # wscale[g][k] * go
                dp32[ch, valid] += (w * scale) * de.astype(F32)               # gpix * (...), signed; a repeat adds
    loss = F32(total / F32(G)) if G > 1 else total
    grad, grad32 = (np.ascontiguousarray(a.reshape(C, B, HW).transpose(1, 0, 2)).reshape(B, C, 1, HW)
                    for a in (dp, dp32))
    grad.setflags(write=False)
    grad32.setflags(write=False)
    return Expected(loss, grad, exact, differ / max(pairs, 1), len(weights), grad32)


@functools.lru_cache(maxsize=2)
def expected_binary(spec):
    """oracle.losses_ref.binary_lovasz (per image, classes=[1], sum(loss * valid) / (sum valid + 0.001)) with the
    designed ranks of channel 1; the gradient in fp64 from the fp32 Jaccard steps and the fp32 denominator"""
    d = build(spec)
    B, HW = spec.B, spec.HW
    lab = d.lab.reshape(B, HW)
    valid = (lab.sum(1) > 0).astype(F32)
    denom = F32(valid.sum(dtype=F32) + F32(0.001))
    total = F32(0.0)
    grad = np.zeros((B, 2, HW), F64)
    grad32 = np.zeros((B, 2, HW), F32)
    differ = pairs = 0
    for b in range(B):
        fg = (lab[b] == 1).astype(F32)
        r = d.rank[1, b * HW:(b + 1) * HW]
        inv = np.empty(HW, np.int64)
        inv[r] = np.arange(HW)
        jg = lovasz_grad(fg[inv])
        a, c = _diversity_counts(jg)
        differ, pairs = differ + a, pairs + c
        li = F32(np.dot(design_errors(spec, HW, np.arange(HW)), jg.astype(F64)))
        total = F32(total + li * valid[b])
        sign = np.where(fg > 0, -1.0, 1.0)
        grad[b, 1] = sign * jg[r].astype(F64) * float(valid[b]) / float(denom)
        grad32[b, 1] = ((sign.astype(F32) * jg[r]) * F32(valid[b] / denom)) * UPSTREAM   # lovasz_bwd_kernel's order
    grad, grad32 = grad.reshape(B, 2, 1, HW), grad32.reshape(B, 2, 1, HW)
    grad.setflags(write=False)
    grad32.setflags(write=False)
    return Expected(F32(total / denom), grad, False, differ / max(pairs, 1), B, grad32)


def check_grad(grad, ref64, exact):
    """the gradient bound of the designed cases, at every element and without an absolute term: exactly 0 where the
    fp64 reference (upstream included) is 0; equal to it where `exact`; else within K_ROUND * 2^-24 * |ref|.  Returns
    the largest error in units of 2^-24 * |ref|."""
    grad, ref64 = np.asarray(grad), np.asarray(ref64)
    assert grad.dtype == F32 and ref64.dtype == F64 and grad.shape == ref64.shape
    zero = ref64 == 0
    assert np.all(grad[zero] == 0), 'a non-zero gradient where the reference is exactly 0'
    nz = ~zero
    ref = ref64[nz]
    worst = float((np.abs(grad[nz].astype(F64) - ref) / (ULP * np.abs(ref))).max()) if ref.size else 0.0
    if exact:
        assert np.array_equal(ref64.astype(F32).astype(F64), ref64), 'the reference is not exact in fp32'
        assert np.array_equal(grad, ref64.astype(F32)), f'not exact: up to {worst:.3f} x 2^-24 |ref|'
    assert worst <= K_ROUND, f'{worst:.3f} x 2^-24 |ref| > K_ROUND = {K_ROUND}'
    return worst


def onehot(spec):
    """dense [B, C, 1, HW] target whose argmax is the label (C >= 2, no void)"""
    d = build(spec)
    t = np.zeros((spec.B, spec.C, 1, spec.HW), F32)
    np.put_along_axis(t, d.lab[:, None], 1.0, 1)
    return t


# ---- the cases ---------------------------------------------------------------------------------------------------
def _s(*a, **k):
    return Spec(*a, **k)


GENERAL = [
    # tile rounds: T = 65 per image (second round of the row scan / segsum), T = 129 for the batch (third round)
    _s('rounds_img', 2, 1, 131073, classes=(1,), per_image=True),
    _s('rounds_batch', 2, 1, 131073, classes=(1,), per_image=False),
    _s('rounds_hinge', 1, 1, 131073, mode='hinge', classes=(1,), per_image=True),
    # void pixels at depth: nvalid on both sides of the 64-tile edge, one valid pixel (the last), whole void tiles
    _s('void_131072', 1, 1, 264193, classes=(1,), ignore=255, void='runs:131072'),
    _s('void_131073', 1, 1, 264193, classes=(1,), ignore=255, void='runs:131073'),
    _s('void_one', 1, 1, 264193, classes=(1,), ignore=255, void='last:1'),
    # grid stride of prep / bwd (1,048,576) and of the count kernel (16,384 per group)
    _s('grid_one', 1, 1, 1048583, classes=(1,)),
    _s('grid_img', 3, 2, 349623, classes='all', per_image=True),
    # chunks by size
    _s('chunk2_all', 1, 3, 1398102, classes='all'),
    _s('chunk2_present', 1, 3, 1398102, classes='present', absent=(0, 2)),
    _s('chunk2_list', 1, 3, 1398102, classes=(1, 0, 1)),
    _s('chunk1_all', 1, 2, 2097153, classes='all'),
    _s('chunk1_present', 1, 2, 2097153, classes='present', absent=(0, 1)),
    _s('chunk1_list', 1, 2, 2097153, classes=(1, 1)),
    _s('chunk7_all', 3, 8, 174763, classes='all', per_image=True),
    _s('chunk7_present', 3, 8, 174763, classes='present', per_image=True, absent=(1, 7)),
    _s('chunk7_list', 3, 8, 174763, classes=(0, 1, 2, 3, 4, 5, 6, 0), per_image=True),
    # many groups
    _s('groups_257', 257, 2, 5, classes='all', per_image=True),
    _s('groups_max', 1285, 51, 2, classes='all', per_image=True),
]
LENGTH_BOUND = _s('length_bound', 1, 1, 1 << 24, classes=(1,))
BINARY = [
    _s('bin_rounds', 2, 2, 131073, classes=(1,), per_image=True),
    _s('bin_grid', 1, 2, 1048583, classes=(1,), per_image=True),
    _s('bin_17', 17, 2, 5, classes=(1,), per_image=True, nofg=3),
    _s('bin_33', 33, 2, 5, classes=(1,), per_image=True, nofg=20),
]
BY_NAME = {s.name: s for s in GENERAL + BINARY + [LENGTH_BOUND]}

# what each case is there to cross: name -> predicate on the spec
CROSSES = {
    'rounds_img': lambda s: tiles(s.L) == SCAN_ROUND + 1,
    'rounds_batch': lambda s: tiles(s.L) == 2 * SCAN_ROUND + 1,
    'rounds_hinge': lambda s: tiles(s.L) == SCAN_ROUND + 1,
    'void_131072': lambda s: tiles(s.L) > 2 * SCAN_ROUND and 131072 == SCAN_ROUND * TILE,
    'void_131073': lambda s: tiles(s.L) > 2 * SCAN_ROUND and 131073 == SCAN_ROUND * TILE + 1,
    'void_one': lambda s: tiles(s.L) > 2 * SCAN_ROUND,
    'grid_one': lambda s: GRID_SPAN < s.B * s.HW < GRID_SPAN + 256 and s.L > COUNT_CAP > COUNT_SPAN,
    'grid_img': lambda s: GRID_SPAN < s.B * s.HW < GRID_SPAN + 512 and s.HW > COUNT_CAP and s.HW % 256 != 0,
    'chunk2_all': lambda s: chunk_classes(s.B * s.HW, s.K) == 2 and s.K == 3,
    'chunk2_present': lambda s: chunk_classes(s.B * s.HW, s.K) == 2 and s.K == 3,
    'chunk2_list': lambda s: chunk_classes(s.B * s.HW, s.K) == 2 and s.K == 3,
    'chunk1_all': lambda s: chunk_classes(s.B * s.HW, s.K) == 1 and s.K == 2,
    'chunk1_present': lambda s: chunk_classes(s.B * s.HW, s.K) == 1 and s.K == 2,
    'chunk1_list': lambda s: chunk_classes(s.B * s.HW, s.K) == 1 and s.K == 2,
    'chunk7_all': lambda s: chunk_classes(s.B * s.HW, s.K) == 7 and s.K == 8 and s.G == 3,
    'chunk7_present': lambda s: chunk_classes(s.B * s.HW, s.K) == 7 and s.K == 8 and s.G == 3,
    'chunk7_list': lambda s: chunk_classes(s.B * s.HW, s.K) == 7 and s.K == 8 and s.G == 3,
    'groups_257': lambda s: s.G == FINAL_GROUPS + 1,
    'groups_max': lambda s: s.G * s.K == MAX_S,
    'length_bound': lambda s: s.L == MAX_L,
    'bin_rounds': lambda s: tiles(s.HW) == SCAN_ROUND + 1,
    'bin_grid': lambda s: GRID_SPAN < s.B * s.HW < GRID_SPAN + 256,
    'bin_17': lambda s: s.B == BIN_FINAL_IMAGES + 1,
    'bin_33': lambda s: s.B == 2 * BIN_FINAL_IMAGES + 1,
}


# ---- the fused softmax: probes on an exactly one-hot background ---------------------------------------------------
# The softmax's errors cannot be designed to the bit, so these cases follow the probe principle: every pixel but 16
# carries logits +60 on its label's class and -60 elsewhere.  exp(-120) / (1 + ...) is below the smallest fp32
# subnormal and 1 / (1 + 2 exp(-120)) rounds to 1, so p is exactly one-hot, every class error is exactly 0 and so is
# the gradient.  The 16 probes carry drawn logits whose errors are 2e-3 apart in every class on the fp64 softmax.
@dataclass(frozen=True)
class ProbeCase:
    spec: Spec
    x: np.ndarray          # [B, C, 1, HW] f32 logits
    lab: np.ndarray        # [B, 1, HW] int64
    sites: Tuple[int, ...]     # flat pixel indices b * HW + p of the probes


SOFTMAX_PROBES = {
    'sm_chunk2': Spec('sm_chunk2', 1, 3, 1398102, mode='softmax', classes='all'),
    'sm_img': Spec('sm_img', 3, 2, 349623, mode='softmax', classes='all', per_image=True),
}
PROBE_GAP = 2e-3           # asked: 1e-3; the margin covers the fp32 rounding of p


def planes(a, spec):
    """[B, C, 1, HW] -> [C, B*HW]"""
    return np.asarray(a).reshape(spec.B, spec.C, spec.HW).transpose(1, 0, 2).reshape(spec.C, spec.B * spec.HW)


def probe_sites(spec):
    N = spec.B * spec.HW
    s = {0, 255, 256, TILE - 1, TILE, GRID_SPAN - 1, GRID_SPAN, N - 1}    # N - 1 | 0: also the chunk boundary's pixels
    for b in range(1, spec.B):
        s |= {b * spec.HW - 1, b * spec.HW}
    for extra in (63, 64, COUNT_SPAN - 1, COUNT_SPAN, 65535, 65536, 2 * TILE - 1, 2 * TILE):
        if len(s) < 16:
            s.add(extra)
    assert len(s) == 16
    return tuple(sorted(s))


def _probe_gap(z, lab):
    """least distance between two probe errors of one class, or to the background's 0, on the fp64 softmax"""
    p = np.exp(z.astype(F64) - z.max(0, keepdims=True))
    p /= p.sum(0, keepdims=True)
    gap = np.inf
    for c in range(z.shape[0]):
        err = np.sort(np.abs((lab == c).astype(F64) - p[c]))
        gap = min(gap, err[0], np.diff(err).min())
    return gap


@functools.lru_cache(maxsize=None)
def softmax_probe_case(name):
    spec = SOFTMAX_PROBES[name]
    B, C, HW = spec.B, spec.C, spec.HW
    N = B * HW
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lab = rng.integers(0, C, N)
    x = np.full((C, N), -60.0, F32)
    x[lab, np.arange(N)] = 60.0
    sites = probe_sites(spec)
    for _ in range(1000):       # redraw until the probes' errors are PROBE_GAP apart in every class
        z = (rng.standard_normal((C, 16)) * 1.5).astype(F32)
        if _probe_gap(z, lab[list(sites)]) >= PROBE_GAP:
            break
    else:
        raise AssertionError('no draw of probe logits is PROBE_GAP apart')
    x[:, list(sites)] = z
    x = np.ascontiguousarray(x.reshape(C, B, HW).transpose(1, 0, 2)).reshape(B, C, 1, HW)
    lab = lab.reshape(B, 1, HW)
    x.setflags(write=False)
    lab.setflags(write=False)
    return ProbeCase(spec, x, lab, sites)


@functools.lru_cache(maxsize=None)
def softmax_probe_expected(name):
    """(loss, gradient) of lovasz_ref.lovasz on the fused-softmax case"""
    case = softmax_probe_case(name)
    s = case.spec
    loss, grad = lovasz_ref.lovasz(case.x, case.lab, 'softmax', s.classes_arg, s.per_image, None)
    grad.setflags(write=False)
    return loss, grad


def probe_upstream(grad):
    """the power of two that puts the largest gradient entry into [2^-8, 2^-7)"""
    return 2.0 ** (-8 - int(np.floor(np.log2(float(np.abs(grad).max())))))
