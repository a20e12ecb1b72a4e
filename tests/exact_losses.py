"""Designed operands and fp64 references for the loss kernels (csrc/seglosses.hip, and the BCE-mean / consistency
kernels of csrc/eltwise.hip) at the sizes where their launch code takes another path.  No GPU here: the host file
test_losses_geometry_host.py proves the designs, test_losses_geometry.py runs them on the device.

The yardsticks are the fp64 restatements of test_losses_ext_host.py (pinned there to the reference's golden vectors)
plus bce_mean64 and consistency64 below, the fp64 form of oracle/losses_ref.py.  Nothing is compared with another
kernel of ours.

Probe principle.  A scalar that is a mean over 270,000 pixels does not notice one lost pixel at rtol 2e-5.  So in a
probe case every pixel but K <= 16 is *background*: an operand on which the loss term is exactly 0 in fp32 (and at
most 2^-60 of the total in fp64).  The K probes carry real values and sit where an index can go wrong: the ends of a
wavefront and a block, the last element of the first round of every grid-stride loop and the first of the second, the
sample boundary, the last element.  The scalar is then the sum of the probes alone, each probe weighs many times the
tolerance, and their contributions differ pairwise by more than 1 %, so a dropped, doubled or swapped probe fails.
"""
import functools

import numpy as np
import torch

from test_losses_ext_host import (bce64, binary_entropy64, ce64, dice_logits64, dice_prob64, entropy64, focal64,
                                  nfl64, ohem64, ohem_state64, smooth64)

F64 = torch.float64

# ---- the launch geometry, as literals (the tests do not parse the kernels) ---------------------------------------
RED_SPAN = 256 * 1024     # seglosses.hip / eltwise.hip: RED_THREADS * RED_BLOCKS, one round of a reduction
GRID_SPAN = 256 * 4096    # common.h ssseg_grid_cap(): 256 threads * the default grid cap of ssseg_grid
PLANE_SPAN = 256 * 64     # seglosses.hip:17: RED_THREADS * PLANE_CHUNKS, one round of a per-plane reduction
PLANE_BWD_SPAN = 256 * 256  # seglosses.hip:877,931: nfl_bwd / dicep_bwd launch at most 256 blocks per plane
FINAL_SPAN = 256 * 256    # the *_final kernels loop nparts = ceil(n / 256) over 256 threads: second round at n > 65,536
PAD = 2.0 ** -60          # the background's share of a scalar, at the most

ALPHA, GAMMA = 0.25, 2.0          # FocalLoss defaults
CONS_THR = 0.7


# ---- fp64 restatements added here --------------------------------------------------------------------------------
def bce_mean64(x, t):
    """oracle/losses_ref.py bce_logits_mean"""
    return bce64(x, t, 'mean')


def consistency64(s, t, thr):
    """oracle/losses_ref.py consistency -> (loss, mean of the confidence mask, number of confident pixels)"""
    ps, pt = torch.sigmoid(s), torch.sigmoid(t)
    cm = (pt.max(1)[0] > thr).to(s.dtype)
    return (((ps - pt) ** 2).sum(1) * cm).sum() / cm.sum(), cm.mean(), int(cm.sum())


# ---- a case ------------------------------------------------------------------------------------------------------
class Case:
    """x, t: fp32 operands (t None for the one-operand losses); xb, tb: the same with every probe replaced by
    background; sites: numpy indices of the probes into x; edge: which launch threshold the shape crosses."""

    def __init__(self, name, family, x, t=None, xb=None, tb=None, sites=(), kw=None, edge=None):
        self.name, self.family, self.x, self.t, self.xb, self.tb = name, family, x, t, xb, tb
        self.sites, self.kw, self.edge = list(sites), dict(kw or {}), edge
        for a in (x, t, xb, tb):
            if a is not None:
                a.setflags(write=False)

    @property
    def npix(self):
        return self.x.shape[0] * int(np.prod(self.x.shape[2:]))

    @property
    def hw(self):
        return int(np.prod(self.x.shape[2:]))


FLAT = ('focal', 'bce_mean', 'bce_sum', 'bce_none', 'bent')  # one thread per element; the others: one per pixel


def fn(case):
    """the loss of a case as a callable on (x, t) tensors of any floating dtype"""
    f, kw = case.family, case.kw
    return {
        'ce': lambda x, t: ce64(x, t, 'mean'),
        'ce_none': lambda x, t: ce64(x, t, 'none'),
        'ohem': lambda x, t: ohem64(x, t, kw.get('thres'), kw.get('min_kept')),
        'focal': lambda x, t: focal64(x, t, ALPHA, GAMMA),
        'bce_mean': bce_mean64,
        'bce_sum': lambda x, t: bce64(x, t, 'sum'),
        'bce_none': lambda x, t: bce64(x, t, 'none'),
        'bent': lambda x, t: binary_entropy64(x),
        'ent': lambda x, t: entropy64(x),
        'nfl': lambda x, t: nfl64(x, t, 0.0)[0],
        'dice': dice_logits64,
        'dicep': dice_prob64,
        'logdicep': lambda x, t: dice_prob64(x, t, True, kw.get('gamma')),
        'cons': lambda x, t: consistency64(x, t, CONS_THR)[0],
    }[f]


def _tt(a, dtype):
    return None if a is None else torch.from_numpy(np.array(a)).to(dtype)   # a copy: the operands are read-only


def evaluate(case, dtype, w=None, x=None, t=None):
    """loss and d (loss * w).sum() / d x at `dtype` on the CPU -> numpy (loss, grad or None without w)"""
    xs = _tt(case.x if x is None else x, dtype).requires_grad_(w is not None)
    ts = _tt(case.t if t is None else t, dtype)
    loss = fn(case)(xs, ts)
    if w is None:
        return loss.detach().numpy(), None
    (loss * torch.as_tensor(np.asarray(w, np.float32)).to(dtype)).sum().backward()
    return loss.detach().numpy(), xs.grad.numpy()


def _w0(case, loss_shape):
    """the unscaled weight of the backward: 1 for a scalar, a fixed pattern in [0.5, 1.5) otherwise"""
    if loss_shape == ():
        return np.float32(1.0)
    n = int(np.prod(loss_shape))
    return (0.5 + (np.arange(n, dtype=np.int64) * 37 % 64).astype(np.float32) / 64).reshape(loss_shape)


@functools.lru_cache(maxsize=3)
def ref64(case):
    """(loss64, grad64, w): the fp64 loss, the weight w (fp32) of the backward and the fp64 gradient of
    (loss * w).sum().  w is a fixed pattern times the power of two that puts the largest |gradient| G into
    [2^-8, 2^-7).  Why: with w = 1 a mean over a million pixels leaves every gradient entry under GRAD_TOL's atol of
    2e-8 and the comparison says nothing.  And an entry that cancels to ~0 (p (log p + H) near p = 1/2) carries the
    fp32 rounding of its O(1) terms, about 1e-6 G whatever its own size (measured on the CPU's fp32 form: 6.7e-7 G),
    so G must stay below 2e-8 / 1e-6 = 0.02 for atol to cover it, with a factor 2.5 to spare at G < 2^-7.  The
    comparison is then GRAD_TOL's rtol on every entry above 1e-4 and 2e-8 <= 5.2e-6 G in absolute terms below."""
    xs, ts = _tt(case.x, F64).requires_grad_(True), _tt(case.t, F64)
    loss = fn(case)(xs, ts)
    w0 = _w0(case, tuple(loss.shape))
    (loss * torch.as_tensor(w0).to(F64)).sum().backward()
    loss, g0 = loss.detach().numpy(), xs.grad.numpy()
    fin = np.abs(g0[np.isfinite(g0)])
    gmax = float(fin.max()) if fin.size else 0.0
    # (a gradient that is rounding noise throughout, as on saturated one-hot predictions, is left unscaled)
    s = float(2.0 ** np.floor(np.log2(2.0 ** -7 / gmax))) if gmax > 2.0 ** -40 else 1.0
    return loss, g0 * s, (w0 * np.float32(s)).astype(np.float32)


# ---- probe positions ---------------------------------------------------------------------------------------------
def positions(n, per_sample=None):
    """the flat positions (< n) at which an index can go wrong; per_sample: the size of one sample, for the last
    element of sample 0 and the first of sample 1"""
    pos = [0, 63, 64, 255, 256, 65535, 65536, 262143, 262144, 262145, n - 1]
    if per_sample is not None and per_sample < n:
        pos += [per_sample - 1, per_sample]
    return sorted({p for p in pos if 0 <= p < n})


def plane_positions(hw):
    return [p for p in (0, 63, 64, 255, 256, 16383, 16384, 16385, hw - 1) if p < hw]


def _targets(rng, k, lo, hi):
    """k draws from U(lo, hi), a draw within 2 % of an earlier one rejected"""
    out = []
    while len(out) < k:
        v = float(rng.uniform(lo, hi))
        if all(abs(v - u) > 0.02 * max(v, u) for u in out):
            out.append(v)
    return out


def _mean_range(n):
    """per-probe terms v with v / n >= 100 * (2e-5 * total + 1e-7) for 16 probes: v >= 1e-5 n + 2e-3 sum(v).  With
    v in [1.3, 2.9] * 1e-5 n the sum is below 46.4e-5 n, and 1e-5 n + 0.093e-5 n < 1.3e-5 n."""
    return 1.3e-5 * n, 2.9e-5 * n


def _bisect(f, target, lo, hi):
    """s in [lo, hi] with f(s) = target, f monotone"""
    up = f(hi) > f(lo)
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if (f(mid) < target) == up:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _px(shape):
    """views [B, C, HW] of fresh fp32 arrays of `shape`"""
    a = np.zeros(shape, np.float32)
    return a, a.reshape(shape[0], shape[1], -1)


def _site(q, hw):
    return (q // hw, slice(None), q % hw)


# ---- builders: softmax family ------------------------------------------------------------------------------------
def _softmax_bg(shape, mag):
    """background: the true class (q mod C) at +mag, the others at -mag; one-hot target"""
    B, C, HW = shape[0], shape[1], int(np.prod(shape[2:]))
    x, xv = _px(shape)
    t, tv = _px(shape)
    cls = (np.arange(B * HW) % C).reshape(B, HW)
    xv[:] = -mag
    for c in range(C):
        xv[:, c][cls == c] = mag
        tv[:, c][cls == c] = 1
    return x, xv, t, tv, HW


def build_ce(name, family, shape, seed, kw=None):
    """CE / OHEM probes: CE = v at the probe (the other classes' logits U(-2, 2), the true one set for it)"""
    rng = np.random.default_rng(seed)
    x, xv, t, tv, HW = _softmax_bg(shape, 30.0)
    xb, tb = x.copy(), t.copy()
    C, npix = shape[1], shape[0] * HW
    pos = positions(npix, HW)
    lo, hi = _mean_range(npix) if family != 'ohem' else (3.0, 8.0)
    sites = []
    for q, v in zip(pos, _targets(rng, len(pos), lo, hi)):
        b, _, p = s = _site(q, HW)
        k = int(rng.integers(C))
        logit = rng.uniform(-2, 2, C)
        others = np.delete(logit, k)
        logit[k] = np.log(np.exp(others).sum()) - np.log(np.expm1(v))
        xv[b, :, p] = logit
        tv[b, :, p] = np.eye(C)[k]
        sites.append(s)
    return Case(name, family, x, t, xb, tb, [(b, slice(None)) + np.unravel_index(p, shape[2:]) for b, _, p in sites],
                kw, 'red')


def build_ent(name, shape, seed):
    """entropy probes: a random direction scaled so that the pixel's entropy is (1 - 0.012 j) ln C: the term cannot
    exceed ln C, so the probes sit as high as they can while staying 1 % apart"""
    rng = np.random.default_rng(seed)
    x, xv, _, _, HW = _softmax_bg(shape, 60.0)
    xb = x.copy()
    C, npix = shape[1], shape[0] * HW
    pos = positions(npix, HW)

    def ent(z):
        z = z - z.max()
        p = np.exp(z) / np.exp(z).sum()
        return float(-(p * np.log(p)).sum())
    sites = []
    for q, j in zip(pos, rng.permutation(len(pos))):
        b, _, p = _site(q, HW)
        r = rng.normal(size=C)
        r /= r.max() - r.min() if C > 1 else 1.0
        s = _bisect(lambda s: ent(s * r), (1 - 0.012 * j) * np.log(C), 0.0, 32.0) if j else 0.0
        xv[b, :, p] = s * r + rng.uniform(-1, 1)
        sites.append((b, slice(None)) + np.unravel_index(p, shape[2:]))
    return Case(name, 'ent', x, None, xb, None, sites, None, 'red')


# ---- builders: element-wise family -------------------------------------------------------------------------------
def build_flat(name, family, shape, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    per = n // shape[0]
    pos = positions(n, per)
    t = (np.arange(n) % 2).astype(np.float32)
    if family == 'bent':
        # -80: sigmoid is 1.8e-35, a normal fp32 number, and 1 - p is exactly 1: the term is -1.4e-33 (at -40 it
        # would be -1.7e-16, 4e-11 of the total over 800,000 elements); positive values are where the reference NaNs
        x = np.full(n, -80.0, np.float32)
        t = None
    else:
        mag = 30.0 if family == 'focal' else 60.0
        x = np.where(t > 0, mag, -mag).astype(np.float32)
    xb, tb = x.copy(), None if t is None else t.copy()
    if family == 'bent':
        h = lambda a: -(a * np.log(a) + (1 - a) * np.log(1 - a))   # noqa: E731
        sig = lambda v: 1 / (1 + np.exp(-v))                          # noqa: E731
        for q, j in zip(pos, rng.permutation(len(pos))):
            s = _bisect(lambda s: h(sig(s)), (1 - 0.012 * j) * np.log(2), 0.0, 5.0) if j else 0.0
            x[q] = s * (1 if rng.random() < 0.5 else -1)
    else:
        lo, hi = (1.0, 4.0) if family == 'bce_sum' else _mean_range(n)
        for q, v in zip(pos, _targets(rng, len(pos), lo, hi)):
            tq = float(rng.integers(2))
            if family == 'focal':
                # the term is ~ alpha_t * |x| on a confident wrong answer
                if tq == 1 and v / ALPHA > 80:
                    tq = 0.0
                v = v / (ALPHA if tq else 1 - ALPHA)
            x[q], t[q] = (-v if tq else v), tq
    rs = lambda a: None if a is None else a.reshape(shape)   # noqa: E731
    return Case(name, family, rs(x), rs(t), rs(xb), rs(tb), [np.unravel_index(q, shape) for q in pos], None, 'red')


# ---- builders: consistency ---------------------------------------------------------------------------------------
def build_cons(name, shape, seed, confident_bg):
    """x = student, t = teacher.  Background: student bit-equal to the teacher (d = 0), the teacher at +60 (every
    background pixel confident) or at -60 (none).  Probes, alternating: confident (one teacher channel >= 2) and not
    confident (every teacher channel -60), the student different in both; sum_c d^2 in [1, C), 1.5 % apart."""
    rng = np.random.default_rng(seed)
    B, C, HW = shape[0], shape[1], int(np.prod(shape[2:]))
    mag = 60.0 if confident_bg else -60.0
    x, xv = _px(shape)
    t, tv = _px(shape)
    xv[:] = mag
    tv[:] = mag
    xb, tb = x.copy(), t.copy()
    sig = lambda v: 1 / (1 + np.exp(-v))   # noqa: E731
    pos, seen, sites, kinds = positions(B * HW, HW), [], [], []
    for i, q in enumerate(pos):
        conf = i % 3 != 2
        while True:
            te = rng.uniform(-3, 3, C) if conf else np.full(C, -60.0)
            if conf:
                te[int(rng.integers(C))] = rng.uniform(2, 4)
            st = rng.uniform(-4, 4, C)
            d2 = float(((sig(st) - sig(te)) ** 2).sum())
            if d2 >= 1.0 and all(abs(d2 - u) > 0.015 * max(d2, u) for u in seen):
                break
        seen.append(d2)
        b, _, p = _site(q, HW)
        xv[b, :, p], tv[b, :, p] = st, te
        sites.append((b, slice(None)) + np.unravel_index(p, shape[2:]))
        kinds.append(conf)
    n_conf = sum(kinds)
    count = B * HW - (len(kinds) - n_conf) if confident_bg else n_conf
    return Case(name, 'cons', x, t, xb, tb, sites, {'kinds': kinds, 'count': count}, 'red')


# ---- builders: per-plane and per-sample reductions ---------------------------------------------------------------
def _distinct(c):
    c = np.abs(np.asarray(c, np.float64))
    c = c[c > 0]
    return all(abs(a - b) > 0.01 * max(a, b) for i, a in enumerate(c) for b in c[i + 1:])


def _reseed(build, seed):
    """the first seed from `seed` on whose case has probe contributions pairwise 1 % apart, each at least 100 x
    (2e-5 |total| + 1e-7), the loss bound of the device test"""
    for s in range(seed, seed + 50):
        case = build(s)
        con = np.abs(contributions(case))
        con = con[:len(con) - case.kw.get('ignored', 0)]
        total = float(np.abs(evaluate(case, F64)[0]).max())
        if _distinct(con) and con.min() >= 110 * (2e-5 * total + 1e-7):
            return case
    raise AssertionError('no seed gives distinct probes')


def build_nfl(name, shape, seed):
    """label > 0 at x = +30, label 0 at x = -30: p_t is exactly 1 in fp32, beta 0.  Probes U(-3, 3) with a random
    label in the first plane, the first plane of sample 1 and the last plane, two of them on ignore-labelled pixels."""
    def build(s):
        rng = np.random.default_rng(s)
        B, C, HW = shape[0], shape[1], int(np.prod(shape[2:]))
        t, tv = _px(shape)
        tv[:] = (np.arange(HW) % 2)[None, None]
        x = np.where(t > 0, 30.0, -30.0).astype(np.float32)
        xv = x.reshape(B, C, HW)
        xb, tb = x.copy(), t.copy()
        where = [(0, p) for p in plane_positions(HW)] + [(C, 0)] + [(B * C - 1, p) for p in plane_positions(HW)[5:]]
        where += [(0, 100), (B * C - 1, 16000)]          # the ignore-labelled ones
        sites = []
        for i, (pl, p) in enumerate(where):
            b, c = divmod(pl, C)
            xv[b, c, p] = rng.uniform(-3, 3)
            tv[b, c, p] = -1 if i >= len(where) - 2 else float(rng.integers(2))
            sites.append((b, c) + np.unravel_index(p, shape[2:]))
        return Case(name, 'nfl', x, t, xb, tb, sites, {'ignored': 2}, 'plane')
    return _reseed(build, seed)


def build_dice(name, shape, seed):
    """class 0 is the background, predicted one-hot (+-60).  Classes >= 1 are in the target only at the probes, at
    least two each per sample, the prediction there one-hot on a class that is right about half the time: I, P and
    T of the classes >= 1 are integers below 10."""
    rng = np.random.default_rng(seed)
    B, C, HW = shape[0], shape[1], int(np.prod(shape[2:]))
    x, xv = _px(shape)
    t, tv = _px(shape)
    xv[:], tv[:, 0] = -60.0, 1.0
    xv[:, 0] = 60.0
    xb, tb = x.copy(), t.copy()
    pp = plane_positions(HW)
    sites = []
    for b, ps in ((0, pp), (B - 1, [0] + pp[5:])):
        for i, p in enumerate(ps):
            k = 1 + i % (C - 1)
            pred = k if rng.random() < 0.5 else int(rng.integers(C))
            xv[b, :, p], tv[b, :, p] = -60.0, 0.0
            xv[b, pred, p], tv[b, k, p] = 60.0, 1.0
            sites.append((b, slice(None)) + np.unravel_index(p, shape[2:]))
    return Case(name, 'dice', x, t, xb, tb, sites, None, 'plane')


def build_dicep(name, family, shape, seed, kw=None):
    """dice_loss / log_dice_loss on probabilities: p = t = 0 but at the probes (p in U(0.1, 0.95), t in {0, 1})"""
    def build(s):
        rng = np.random.default_rng(s)
        B, n = shape[0], int(np.prod(shape[1:]))
        x, t = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        xv, tv = x.reshape(B, n), t.reshape(B, n)
        xb, tb = x.copy(), t.copy()
        pp = plane_positions(n)
        sites = []
        for b, ps in ((0, pp), (B - 1, [0] + pp[5:])):
            for i, p in enumerate(ps):
                xv[b, p], tv[b, p] = rng.uniform(0.1, 0.95), float(i % 3 != 1)
                sites.append((b,) + np.unravel_index(p, shape[1:]))
        return Case(name, family, x, t, xb, tb, sites, kw, 'sample')
    return _reseed(build, seed)


# ---- what each probe weighs --------------------------------------------------------------------------------------
def _drop(case, i):
    x, t = case.x.copy(), None if case.t is None else case.t.copy()
    x[case.sites[i]] = case.xb[case.sites[i]]
    if t is not None:
        t[case.sites[i]] = case.tb[case.sites[i]]
    return x, t


def _only(case, i):
    """the operands cut down to probe i: [1, C, 1, 1] or [1]"""
    s = case.sites[i]
    cut = (lambda a: None if a is None else np.ascontiguousarray(a[s], np.float32).reshape(1, -1, 1, 1))
    return cut(case.x), cut(case.t)


def contributions(case):
    """fp64: what probe i adds to the scalar (for the per-sample losses: the largest change of an output when the
    probe is replaced by background).  OHEM and consistency are means over a count that the test checks exactly, so
    the contribution is the probe's term over that count; a probe that must stay out of the sum (consistency, not
    confident) is given the weight it would have inside."""
    f = case.family
    if f in ('nfl', 'dice', 'dicep', 'logdicep'):
        full, _ = evaluate(case, F64)
        return [float(np.abs(full - evaluate(case, F64, None, *_drop(case, i))[0]).max())
                for i in range(len(case.sites))]
    out = []
    for i in range(len(case.sites)):
        x, t = _only(case, i)
        xs, ts = _tt(x, F64), _tt(t, F64)
        if f == 'ohem':
            v = float(ce64(xs, ts, 'none').sum()) / len(case.sites)
        elif f == 'cons':
            v = float(((torch.sigmoid(xs) - torch.sigmoid(ts)) ** 2).sum()) / case.kw['count']
        elif f in ('ce', 'ent'):
            v = float(fn(case)(xs, ts)) / case.npix
        elif f == 'bce_sum':
            v = float(fn(case)(xs, ts))
        else:
            v = float(fn(case)(xs, ts)) / case.x.size
        out.append(v)
    return out


def background(case, dtype):
    """the scalar of the all-background operands (for the means over a count: the sum the count divides)"""
    f = case.family
    xs, ts = _tt(case.xb, dtype), _tt(case.tb, dtype)
    if f == 'ohem':
        return (ce64(xs, ts, 'none').sum() / len(case.sites)).numpy()
    if f == 'cons':
        return (((torch.sigmoid(xs) - torch.sigmoid(ts)) ** 2).sum() / case.kw['count']).numpy()
    return fn(case)(xs, ts).numpy()


# ---- the probe cases ---------------------------------------------------------------------------------------------
S_RED, S_BATCH, S_PLANE, S_SAMPLE = (1, 3, 521, 521), (3, 2, 301, 307), (2, 3, 131, 131), (2, 2, 95, 97)

_PROBE = {}
for _tag, _shape in (('red', S_RED), ('batch', S_BATCH)):
    _PROBE[f'ce_{_tag}'] = functools.partial(build_ce, f'ce_{_tag}', 'ce', _shape, 11)
    _PROBE[f'ce_none_{_tag}'] = functools.partial(build_ce, f'ce_none_{_tag}', 'ce_none', _shape, 12)
    _PROBE[f'ohem_{_tag}'] = functools.partial(build_ce, f'ohem_{_tag}', 'ohem', _shape, 13,
                                               {'thres': 0.7, 'min_kept': 5})
    _PROBE[f'ent_{_tag}'] = functools.partial(build_ent, f'ent_{_tag}', _shape, 14)
    for _i, _f in enumerate(('focal', 'bce_mean', 'bce_sum', 'bce_none', 'bent')):
        _PROBE[f'{_f}_{_tag}'] = functools.partial(build_flat, f'{_f}_{_tag}', _f, _shape, 20 + _i)
    _PROBE[f'cons_{_tag}'] = functools.partial(build_cons, f'cons_{_tag}', _shape, 30, True)
    _PROBE[f'cons_quiet_{_tag}'] = functools.partial(build_cons, f'cons_quiet_{_tag}', _shape, 31, False)
_PROBE['nfl_plane'] = functools.partial(build_nfl, 'nfl_plane', S_PLANE, 40)
_PROBE['dice_plane'] = functools.partial(build_dice, 'dice_plane', S_PLANE, 41)
_PROBE['dicep_sample'] = functools.partial(build_dicep, 'dicep_sample', 'dicep', S_SAMPLE, 42)
_PROBE['logdicep_sample'] = functools.partial(build_dicep, 'logdicep_sample', 'logdicep', S_SAMPLE, 43, {'gamma': 2.0})
PROBE_CASES = sorted(_PROBE)

# The factor by which every probe outweighs the bound (rtol |total| + atol).  100, but where the term of one element
# cannot be that large: an entropy is at most ln C per pixel (ln 2 / 2 per element for the binary one) and a
# consistency term at most C, all under a mean over > 262,144 elements against LOSS_TOL's atol of 1e-7.
PROBE_FACTOR = {'ent': 20, 'bent': 3, 'cons': 30}


def probe_factor(case):
    if case.family == 'cons':
        return 100 if case.name.startswith('cons_quiet') else PROBE_FACTOR['cons']
    return PROBE_FACTOR.get(case.family, 100)


@functools.lru_cache(maxsize=3)
def probe_case(name):
    return _PROBE[name]()


def crosses(case):
    """does the shape reach the edge it is there for"""
    n_px, n_el, hw = case.npix, case.x.size, case.hw
    if case.edge == 'red':
        n = n_el if case.family in FLAT else n_px
        return n > RED_SPAN and n > FINAL_SPAN and n % 64 != 0
    if case.edge == 'plane':
        return hw > PLANE_SPAN and hw % 64 != 0
    if case.edge == 'sample':
        return n_el // case.x.shape[0] > PLANE_SPAN
    if case.edge == 'grid':
        n = n_el if case.family in FLAT else n_px
        ok = n > GRID_SPAN and n % 256 != 0
        if case.family == 'nfl':
            ok = ok and hw > PLANE_BWD_SPAN
        if case.family in ('dicep', 'logdicep'):
            ok = n_el // case.x.shape[0] > PLANE_BWD_SPAN
        return ok
    return case.edge == 'width'


# ---- the channel-width sweep -------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
SWEEP_HW = ((17, 31), (7, 9))
SWEEP_FAMILIES = ('ce', 'ohem', 'dice', 'ent')


@functools.lru_cache(maxsize=None)
def sweep_case(family, C, hw):
    """plain random logits, a random one-hot target (a soft one for CE)"""
    rng = np.random.default_rng(1000 * C + hw[0])
    shape = (2, C) + tuple(hw)
    x = rng.normal(size=shape).astype(np.float32)
    if family == 'ce':
        z = rng.normal(size=shape)
        t = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(np.float32)
    else:
        t = np.moveaxis(np.eye(C, dtype=np.float32)[rng.integers(C, size=(2,) + tuple(hw))], -1, 1).copy()
    kw = {'thres': 0.7, 'min_kept': 2 * hw[0] * hw[1] // 4} if family == 'ohem' else None
    return Case(f'{family}_c{C}_{hw[0]}x{hw[1]}', family, x, None if family == 'ent' else t, kw=kw, edge='width')


# ---- the second round of the element-wise and backward kernels ---------------------------------------------------
S_GRID = (3, 2, 1, 349_623)
GRID_FAMILIES = ('ce', 'ce_none', 'ohem', 'dice', 'ent', 'focal', 'bent', 'bce_none', 'bce_sum', 'bce_mean', 'cons',
                 'nfl', 'dicep', 'logdicep')


@functools.lru_cache(maxsize=2)
def grid_case(family):
    """ordinary operands at 1,048,869 pixels: logits of magnitude U(0.3, 2.5) with a random sign (no sigmoid or
    softmax saturates and no logit sits on the cancellation at 0), random one-hot / binary targets"""
    rng = np.random.default_rng(GRID_FAMILIES.index(family) + 77)
    shape, C = S_GRID, S_GRID[1]
    x = (rng.uniform(0.3, 2.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    kw = None
    if family in ('ce', 'ce_none', 'ohem', 'dice'):
        t = np.moveaxis(np.eye(C, dtype=np.float32)[rng.integers(C, size=(shape[0],) + shape[2:])], -1, 1).copy()
        if family == 'ohem':
            # thres in the middle of the widest gap between two preds in [0.65, 0.75]: the selection is the same in
            # fp32 and fp64 (the order statistic, the 100,000th smallest pred, is far below it)
            z = x.astype(np.float64)
            pr = np.sort((np.exp(z) * t).sum(1).ravel() / np.exp(z).sum(1).ravel())
            pr = pr[(pr > 0.65) & (pr < 0.75)]
            i = int(np.argmax(np.diff(pr)))
            kw = {'thres': float(0.5 * (pr[i] + pr[i + 1])), 'min_kept': 100000}
    elif family in ('ent', 'bent'):
        t = None
    elif family == 'cons':
        # no teacher logit within 0.05 of logit(CONS_THR) = 0.847: the confidence mask is the same in fp32 and fp64
        mag = rng.uniform(0.3, 2.4, shape)
        t = ((mag + 0.1 * (mag > 0.8)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    elif family == 'nfl':
        t = rng.integers(-1, 2, shape).astype(np.float32)
        t[0] = np.abs(t[0])                               # sample 0 has no ignored pixel
    else:
        t = rng.integers(0, 2, shape).astype(np.float32)
    if family in ('dicep', 'logdicep'):
        x = rng.uniform(0.05, 0.95, shape).astype(np.float32)
        kw = {'gamma': 2.0}
    return Case(f'{family}_grid', family, x, t, kw=kw, edge='grid')


# ---- the OHEM selection design -----------------------------------------------------------------------------------
class OhemDesign:
    """M logit vectors (C = 2: true class 0, the other a_i, pred_i = 1 / (1 + exp(a_i))), vector i at r_i scattered
    pixels; the rest is background with pred exactly 1.0.  Identical inputs give bit-identical preds on the device,
    so the ties are real.  Group sizes 1, 2, 3, 255, 256, 257 and one above 65,536; the fp64 preds are >= 1e-3 apart
    but one pair ~1.2e-6 (>= 100 fp32 ulp) apart whose fp32 keys share the upper three bytes; one pred is below
    2^-20."""
    shape = S_BATCH
    #        pred ~     size
    groups = ((3.1e-7, 3), (0.05, 1), (0.1, 256), (None, 257), (0.15, 2), (0.2, 70000), (0.3, 255), (0.4, 17),
              (0.5, 1000), (0.55, 5), (0.62, 100), (0.8, 40))
    PAIR_GAP = 1.2e-6

    def __init__(self):
        B, C, H, W = self.shape
        HW, npix = H * W, B * H * W
        rng = np.random.default_rng(5)
        a = []
        for p, _ in self.groups:
            if p is None:
                a[-1], upper = self._close_pair(a[-1])
                a.append(upper)
            else:
                a.append(float(np.float32(np.log(1 / p - 1))))
        self.a = a
        self.pred = [1 / (1 + np.exp(ai)) for ai in a]                 # fp64, ascending
        assert all(u < v for u, v in zip(self.pred, self.pred[1:]))
        self.sizes = [r for _, r in self.groups]
        self.cum = np.cumsum(self.sizes).tolist()
        self.npix, self.HW = npix, HW
        x, xv = _px(self.shape)
        t, tv = _px(self.shape)
        xv[:, 0], xv[:, 1], tv[:, 0] = 30.0, -30.0, 1.0
        where = rng.permutation(npix)[:self.cum[-1]]
        lo = 0
        for ai, r in zip(a, self.sizes):
            q = where[lo:lo + r]
            xv[q // HW, 0, q % HW], xv[q // HW, 1, q % HW] = 0.0, ai
            lo += r
        self.x, self.t = x, t
        self.thresholds = (1e-9, 0.25, 0.7)

    @classmethod
    def _close_pair(cls, start):
        """logits (lower, upper pred) near `start`: the lower pred's fp32 key has a low byte in [16, 48], so the upper
        one, PAIR_GAP = 161 ulp above, shares its upper three bytes with a margin for the device's own expf"""
        def key(a):
            p = torch.softmax(torch.tensor([0.0, a], dtype=torch.float32), 0)[0]
            return int(p.numpy().view(np.uint32)), float(p)
        for cand in np.arange(start, start - 1e-3, -1e-6, dtype=np.float64):
            lo = float(np.float32(cand))
            k_lo, p_lo = key(lo)
            up = float(np.float32(np.log(1 / (p_lo + cls.PAIR_GAP) - 1)))
            if 16 <= k_lo & 255 <= 48 and k_lo >> 8 == key(up)[0] >> 8:
                return lo, up
        raise AssertionError('no close pair found')

    def ranks(self):
        """min_kept values: 1, the interior of a group, each cumulative count and one less, npix - 1, 10 npix"""
        ks = {1, self.cum[5] - 1234, self.cum[2] - 100, self.npix - 1, 10 * self.npix, self.cum[-1] + 5}
        for c in self.cum:
            ks.update((c, c - 1))
        return sorted(k for k in ks if k >= 1)

    def expected(self, k, thres):
        """(threshold, kept count, fp64 loss) from the group sizes alone"""
        k = min(max(1, k), self.npix - 1)
        j = int(np.searchsorted(self.cum, k, side='right'))          # the group that holds sorted index k
        val = self.pred[j] if j < len(self.pred) else 1.0
        thr = max(val, thres)
        kept = sum(r for p, r in zip(self.pred, self.sizes) if p < thr)
        num = sum(-np.log(p) * r for p, r in zip(self.pred, self.sizes) if p < thr)
        return thr, kept, (num / kept if kept else float('nan'))


@functools.lru_cache(maxsize=1)
def ohem_design():
    return OhemDesign()
