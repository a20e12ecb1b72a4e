"""GPU: ops.uncertainty_scores (csrc/active.hip) against the fp64 oracle of active_ref.py at the shapes where the launch
changes its path, the designed cases, the bitwise properties and the refusals.

Bound: the larger of 4 x the error of the same stable formula evaluated in fp32 on the CPU against fp64, and an
absolute floor of 1e-6 (about 2 ulp at log 64 = 4.16, the largest possible value).  Every test prints its figures
before it asserts."""
import os
import re

import numpy as np
import pytest
import torch

import active_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu


def _constants():
    src = open(os.path.join(PKG, 'csrc', 'active.hip')).read()
    return {k: int(v) for k, v in re.findall(r'constexpr int (ACT_[A-Z0-9_]+) = (\d+);', src)}


K = _constants()
THREADS, MAX_BLOCKS = K['ACT_THREADS'], K['ACT_MAX_BLOCKS']


PX, CHUNK = K['ACT_PX'], K['ACT_CHUNK']
SWEEP = THREADS * PX                       # pixels one block covers in one sweep
SHAPES = [(1, 2, 1, 1), (3, 2, 1, 3), (2, 3, 5, 7), (2, 19, 33, 31), (1, 64, 16, 17),
          (2, 5, 1, 4 * 37 + 1), (2, 5, 1, 4 * 37),                          # HW = 4k + 1 (scalar loads, tail), 4k
          (2, 2, 1, SWEEP - 1), (2, 2, 1, SWEEP + 1),                        # one block's sweep, just below / above
          (2, 33, 1, SWEEP), (2, 20, 1, SWEEP + 3),
          (1, 2, 1, 2 * MAX_BLOCKS * SWEEP + 5),                             # every block of the image loops twice
          (1, 11, 1, 2 * MAX_BLOCKS * SWEEP + 4)]
# both sides of every channel bucket: the whole pixel in registers for C <= 2 and C <= 4, then chunks of CHUNK channels
SHAPES += [(2, c, 3, 7) for c in sorted({2, 3, 4, 5} | {k * CHUNK + d for k in range(1, 64 // CHUNK) for d in (0, 1)}
                                        | {63, 64})]


def logits(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * 3


def device_scores(x, dev):
    from ssseg import ops
    return ops.uncertainty_scores(x.to(dev))


def bound(x):
    ref = R.scores(x.numpy())
    return ref, np.maximum(4 * np.abs(R.scores(x.numpy(), np.float32) - ref), 1e-6)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_scores_match_fp64_oracle(hip_device, shape):
    x = logits(shape, seed=sum(shape))
    got = device_scores(x, hip_device).cpu().numpy().astype(np.float64)
    ref, tol = bound(x)
    err = np.abs(got - ref)
    print(shape, 'max abs error', err.max(0), 'bound', tol.min(0), 'relative', (err / np.abs(ref)).max())
    assert got.shape == (shape[0], 3)
    assert (err <= tol).all()


def test_geometry_constants_are_the_launch_s():
    assert THREADS % 64 == 0 and MAX_BLOCKS >= 1 and PX == 4 and 64 % CHUNK == 0


def test_all_logits_equal(hip_device):
    for C in (2, 19, 64):
        got = device_scores(torch.full((2, C, 5, 7), 1.25), hip_device).cpu().numpy().astype(np.float64)
        want = np.array([np.log(C), 1 - 1 / C, 1.0])
        print(C, got[0], want)
        assert (np.abs(got - want) <= 1e-6).all()
        assert (got[:, 2] == 1.0).all()


def test_saturated_pixels_score_exactly_zero(hip_device):
    for C in (2, 19, 33):
        x = torch.zeros(2, C, 3, 5)
        x[:, C // 2] = 200.0
        got = device_scores(x, hip_device).cpu().numpy()
        print(C, got)
        assert not np.isnan(got).any() and (got == 0.0).all()
        # what the reference's p * log(p) gives on these logits
        p = torch.softmax(x, 1)
        assert torch.isnan(-(p * torch.log(p)).sum(1).mean())


def test_tied_maximum(hip_device):
    x = torch.full((1, 7, 4, 4), -100.0)
    x[:, 2] = 50.0
    x[:, 5] = 50.0
    got = device_scores(x, hip_device).cpu().numpy().astype(np.float64)
    print(got)
    assert got[0, 2] == 1.0 and got[0, 1] == 0.5 and abs(got[0, 0] - np.log(2)) <= 1e-6


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('shape', [(3, 19, 33, 31), (3, 2, 1, SWEEP * 3 + 1), (3, 5, 8, 12), (3, 40, 8, 8)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_batch_independence_and_reproducibility(hip_device, shape):
    x = logits(shape, seed=7)
    x[2] = x[0]                                                        # two identical images in one batch
    xd = x.to(hip_device)
    from ssseg import ops
    full = ops.uncertainty_scores(xd)
    assert np.array_equal(_bits(full), _bits(ops.uncertainty_scores(xd)))              # two runs
    for b in range(3):
        assert np.array_equal(_bits(full[b:b + 1]), _bits(ops.uncertainty_scores(xd[b:b + 1]))), b
    assert np.array_equal(_bits(full[0]), _bits(full[2]))
    # a batch of another size, and an image at an address that rules the wide loads out
    assert np.array_equal(_bits(full[1:]), _bits(ops.uncertainty_scores(xd[1:])))
    flat = torch.empty(xd[1].numel() + 1, device=hip_device)
    flat[1:] = xd[1].reshape(-1)
    assert np.array_equal(_bits(full[1:2]), _bits(ops.uncertainty_scores(flat[1:].view(1, *shape[1:]))))


def test_graph_replay_equals_eager(hip_device):
    from ssseg import ops
    x = logits((2, 19, 16, 17), seed=3).to(hip_device)
    eager = ops.uncertainty_scores(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.uncertainty_scores(x)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.uncertainty_scores(x)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(eager))


def test_refusals_and_conversions(hip_device):
    from ssseg import native as N
    from ssseg import ops
    for C in (1, 65):
        with pytest.raises(ValueError, match='channels'):
            ops.uncertainty_scores(torch.zeros(1, C, 4, 4, device=hip_device))
        x = torch.zeros(1, C, 16, device=hip_device)
        out = torch.zeros(1, 3, device=hip_device)
        ws = torch.zeros(4096, dtype=torch.uint8, device=hip_device)
        assert N.lib().ssseg_uncertainty_scores(x.data_ptr(), 1, C, 16, out.data_ptr(), ws.data_ptr(), 4096, None) == -1
    with pytest.raises((RuntimeError, ValueError), match='HIP device tensor'):
        ops.uncertainty_scores(torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError):
        ops.uncertainty_scores(torch.zeros(4, 4, device=hip_device))
    # the Python layer converts: a channels-last view (what the models' heads return), bf16 and fp64 logits
    x = logits((2, 5, 6, 7), seed=11)
    want = _bits(ops.uncertainty_scores(x.to(hip_device)))
    cl = x.to(hip_device).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and np.array_equal(_bits(ops.uncertainty_scores(cl)), want)
    assert np.array_equal(_bits(ops.uncertainty_scores(x.double().to(hip_device))), want)
    xb = x.bfloat16()
    assert np.array_equal(_bits(ops.uncertainty_scores(xb.to(hip_device))),
                          _bits(ops.uncertainty_scores(xb.float().to(hip_device))))
