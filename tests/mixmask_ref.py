"""Plain torch / numpy CPU restatements of the ClassMix and CutMix masks (csrc/mixmask.hip), and the designed inputs
the host and GPU tests share.  Nothing here touches the device or the package under test."""
import numpy as np
import torch


# ---- ClassMix --------------------------------------------------------------------------------------------------------
def labels(logits):
    """[B,C,H,W] -> [B,H,W] int64: argmax over the channels in fp32, the first maximum wins, NaN counts as the maximum
    (the first NaN wins) -- written out, not taken from torch.argmax"""
    x = logits.detach().float().cpu().numpy()
    B, C, H, W = x.shape
    lab = np.zeros((B, H, W), np.int64)
    best = x[:, 0].copy()
    for c in range(1, C):
        v = x[:, c]
        take = ~np.isnan(best) & ((v > best) | np.isnan(v))
        best = np.where(take, v, best)
        lab = np.where(take, c, lab)
    return torch.from_numpy(lab)


def choose(present, keys_b, half=lambda n: (n + n % 2) // 2):
    """the k = ceil(n/2) classes of the set `present` with the smallest (key, class)"""
    order = sorted(present, key=lambda c: (int(keys_b[c]), c))
    return set(order[:half(len(present))])


def classmix(logits, keys, half=lambda n: (n + n % 2) // 2, use_presence=True):
    """-> mask [B,1,H,W] f32, present [B] int64, chosen [B] int64, n [B], k [B].  `half` and `use_presence` exist so
    that the tests can show a wrong restatement failing the comparison."""
    lab = labels(logits)
    B, C = logits.shape[:2]
    keys = torch.as_tensor(keys).cpu().numpy().astype(np.int64)
    mask = torch.zeros(B, 1, *lab.shape[1:], dtype=torch.float32)
    present, chosen, ns, ks = [], [], [], []
    for b in range(B):
        pres = set(int(c) for c in np.unique(lab[b].numpy())) if use_presence else set(range(C))
        ch = choose(pres, keys[b], half)
        for c in ch:
            mask[b, 0][lab[b] == c] = 1.0
        present.append(sum(1 << c for c in pres))
        chosen.append(sum(1 << c for c in ch))
        ns.append(len(pres))
        ks.append(len(ch))
    return mask, as_words(present), as_words(chosen), ns, ks


def as_words(values):
    """unsigned 64-bit words as the int64 tensor that holds their bits"""
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64).copy())


def popcounts(words):
    return [bin(int(w) & (2 ** 64 - 1)).count('1') for w in words.cpu().tolist()]


def classmix_inputs(C, H, W, dtype=torch.float32, seed=0):
    """(logits [2,C,H,W], keys [2,C]).  Image 0: random logits; pixel q < min(C, HW) belongs to class q outright (every
    class present where C <= HW, so n = C: odd at an odd C); then planted exact ties and NaNs.  Image 1: class C-1
    everywhere (n = 1)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + seed)
    x = torch.randn(2, C, H, W, generator=g)
    x = x.to(dtype).float()              # values the dtype holds exactly: the reference sees what the kernel sees
    HW = H * W
    flat = x.view(2, C, HW)
    # image 0: pixel q < min(C, HW) belongs to class q outright (every class present where C <= HW)
    for q in range(min(C, HW)):
        flat[0, :, q] = -4.0
        flat[0, q, q] = 4.0
    # planted ties on pixels past those: two or more channels share the exact maximum, the first must win
    q0 = min(C, HW)
    if C >= 2 and q0 + 3 <= HW:
        flat[0, :, q0] = 1.0                                   # all channels equal -> class 0
        flat[0, :, q0 + 1] = -1.0
        flat[0, C - 1, q0 + 1] = 2.0
        flat[0, C // 2, q0 + 1] = 2.0                          # tie of C//2 and C-1 -> C//2
        flat[0, C - 1, q0 + 2] = float('nan')                  # NaN counts as the maximum
        if C >= 3:
            flat[0, 1, q0 + 2] = float('nan')                  # the first NaN wins
    only = C - 1
    flat[1] = -3.0
    flat[1, only] = 3.0
    return x.to(dtype), torch.randint(0, 2 ** 31, (2, C), generator=g).to(torch.int32)


# ---- CutMix ----------------------------------------------------------------------------------------------------------
def cutmix_terms(params, H, W, rng):
    """the four products that are rounded, per image, in fp64: H p^u, W p^(1-u), (H-h) v1, (W-w) v2"""
    q = torch.as_tensor(params).detach().cpu().float().numpy().astype(np.float64)
    lo, hi = float(rng[0]), float(rng[1])
    p = lo + (hi - lo) * q[:, 0]
    u, v1, v2 = q[:, 1], q[:, 2], q[:, 3]
    th, tw = H * np.power(p, u), W * np.power(p, 1.0 - u)
    h, w = np.rint(th), np.rint(tw)
    return p, th, tw, (H - h) * v1, (W - w) * v2


def cutmix_boxes(params, H, W, rng):
    """[B,4] int32: top, left, h, w (np.rint rounds half to even)"""
    p, th, tw, tt, tl = cutmix_terms(params, H, W, rng)
    return torch.from_numpy(np.stack([np.rint(tt), np.rint(tl), np.rint(th), np.rint(tw)], 1).astype(np.int32))


def cutmix(params, H, W, rng):
    """-> mask [B,1,H,W] f32, boxes [B,4] int32"""
    boxes = cutmix_boxes(params, H, W, rng)
    mask = torch.zeros(boxes.shape[0], 1, H, W, dtype=torch.float32)
    for b, (top, left, h, w) in enumerate(boxes.tolist()):
        mask[b, 0, top:top + h, left:left + w] = 1.0
    return mask, boxes


RANGE = (0.25, 0.75)
ONE = 1.0 - 2.0 ** -24     # the largest uniform a 24-bit draw gives: v -> 1

# the designed params (B = 8) of the box tests, used with RANGE: (p', u, v1, v2)
DESIGNED = torch.tensor([
    [0.50, 0.50, 0.47, 0.53],      # a box near the centre
    [0.10, 0.30, 0.00, 0.00],      # v = 0: flush to the top-left corner
    [0.90, 0.70, ONE, ONE],        # v -> 1: flush to the bottom-right corner
    [0.30, 0.00, 0.40, 0.60],      # u = 0: h = H, a full-height band
    [0.70, ONE, 0.20, 0.80],       # u -> 1: w = W, a full-width band
    [0.05, 0.55, ONE, 0.00],       # bottom-left
    [0.95, 0.45, 0.00, ONE],       # top-right
    [0.42, 0.37, 0.63, 0.29],
], dtype=torch.float32)


def half_integer_distance(t):
    """distance of every value to the nearest half-integer (k + 0.5)"""
    return np.abs(t - np.floor(t) - 0.5)


def area_gaps(boxes, p, H, W):
    """per box (|h w - H W p|, 0.5 (h + w) + 0.25).  With h = H p^u + d and w = W p^(1-u) + e, |d|, |e| <= 0.5:
    h w - H W p = h e + w d - d e, so the first never exceeds the second."""
    return [(abs(h * w - H * W * pb), 0.5 * (h + w) + 0.25) for (_, _, h, w), pb in zip(boxes.tolist(), p.tolist())]


def fmt_words(words):
    return [hex(int(w) & (2 ** 64 - 1)) for w in words.cpu().tolist()]
