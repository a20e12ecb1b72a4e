"""fp64 torch restatement of the per-sample affine warp (include/ssseg.h, ssseg_affine_warp_fwd) and of the weighted
consistency loss, for tests/test_geo_consistency.py and tests/test_geo_host.py.  Everything here is CPU fp64 and built
from the closed formulas alone: A(theta, s) = [al, be, cx - al cx - be cy; -be, al, cy + be cx - al cy] with
al = cos(theta) / s, be = -sin(theta) / s, cx = (W-1)/2, cy = (H-1)/2, and A^-1 = A(-theta, 1/s)."""
import math

import torch
import torch.nn.functional as F

# the per-sample (theta degrees, zoom) pairs of the suite
PAIRS = [(0.0, 1.0), (17.5, 0.8), (-33.0, 1.25), (45.0, 2.0), (90.0, 1.0), (-7.0, 0.5), (15.0, 0.75), (-15.0, 1.25)]


def mat64(theta_deg, s, H, W):
    th = math.radians(theta_deg)
    al, be = math.cos(th) / s, -math.sin(th) / s
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return torch.tensor([al, be, cx - al * cx - be * cy, -be, al, cy + be * cx - al * cy], dtype=torch.float64)


def mats64(params, H, W):
    """(A, A^-1) as [B, 6] fp64 for a list of (theta, s)."""
    return (torch.stack([mat64(t, s, H, W) for t, s in params]),
            torch.stack([mat64(-t, 1.0 / s, H, W) for t, s in params]))


def coords(mats, H, W):
    """sampling coordinates (sx, sy), each [B, H, W] fp64"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    m = mats.double()[:, :, None, None]
    return m[:, 0] * xs + m[:, 1] * ys + m[:, 2], m[:, 3] * xs + m[:, 4] * ys + m[:, 5]


def warp(x, mats):
    """grid_sample(align_corners=True, padding_mode='zeros') at the coordinates above.  The input gets one more row
    and column of zeros (what the padding mode reads there anyway), so that a 1-pixel axis still has a pixel pitch
    to normalise the coordinates with."""
    B, C, H, W = x.shape
    sx, sy = coords(mats, H, W)
    xp = F.pad(x.double(), (0, 1, 0, 1))
    grid = torch.stack([sx / W * 2 - 1, sy / H * 2 - 1], -1)
    return F.grid_sample(xp, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def valid(mats, H, W):
    sx, sy = coords(mats, H, W)
    return ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).double()


def border_clearance(mats, H, W):
    """the least distance of any sampling coordinate to the borders 0, W-1, H-1 of the validity rule"""
    sx, sy = coords(mats, H, W)
    return float(torch.stack([sx.abs(), (sx - (W - 1)).abs(), sy.abs(), (sy - (H - 1)).abs()]).min())


def consistency_w(s, t, w, thr):
    """(sum d^2 cm w / sum cm w, sum cm w / npix) of fp64 logits s, t [B,C,H,W] and weights w [B,H,W]"""
    ps, pt = torch.sigmoid(s.double()), torch.sigmoid(t.double())
    cm = (pt.max(1)[0] > thr).double() * w.double()
    d2 = ((ps - pt) ** 2).sum(1)
    return (d2 * cm).sum() / cm.sum(), cm.sum() / cm.numel()


def gate_clearance(t, thr):
    """the least distance of the teacher's per-pixel confidence to the threshold"""
    return float((torch.sigmoid(t.double()).max(1)[0] - thr).abs().min())
