"""GPU tests of the general Lovász losses (csrc/lovasz.hip, ssseg_lovasz_gen_*) against the numpy restatement in
tests/lovasz_ref.py and the reference fixtures tests/golden/lovasz_gen_*.npz.

TILE is 2048 sorted elements; the shapes stand on its edges and on the group boundary.  Bounds against lovasz_ref are
those of test_hip_losses.test_lovasz_vs_oracle (the arithmetic is the same): loss rtol 2e-5 / atol 1e-7, gradient
rtol 1e-4 / atol 2e-6 under an upstream scale of 0.7.  Every comparison of per-pixel gradients first asserts on the CPU
that no two valid errors of a segment are equal, so nothing is excluded."""
import functools

import numpy as np
import pytest
import torch

import lovasz_ref
from conftest import golden
from test_lovasz_general_host import EXPECTED, fixture_call

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 23, 29), (2, 5, 32, 33), (1, 4, 64, 32), (1, 2, 2049, 1), (2, 21, 16, 16), (2, 64, 8, 8),
          (4, 3, 1, 1)]
HINGE_SHAPES = [(3, 1, 23, 29), (2, 1, 2049, 1), (4, 1, 1, 1)]
SCALE = np.float32(0.7)
# seeds moved until no segment of the shape holds two equal errors (the precondition of the per-pixel comparisons):
# 2049 two-class probabilities collide in fp32 for the first two seeds
SEED_SHIFT = {(1, 2, 2049, 1): 2}


def class_list(C):
    return sorted({1, C // 2, C - 1})


def void_runs(lab, rng):
    """runs of 255 in lab [B, HW]: a whole tile's worth (2048) in the first image of the 2049-pixel shapes, the third
    single-pixel image, two runs per image elsewhere"""
    B, HW = lab.shape
    if HW == 1:
        lab[2 % B] = 255
    elif HW == 2049:
        lab[0, 1:] = 255
        lab[1:, 100:131] = 255
    else:
        for b in range(B):
            for _ in range(2):
                s = int(rng.integers(0, HW - 2))
                lab[b, s:s + int(rng.integers(2, max(3, HW // 6)))] = 255
    return lab


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=0):
    """(logits x2, host softmax, labels with void runs) of a shape: computed once, never modified"""
    B, C, H, W = shape
    rng = np.random.default_rng(1000 * B + 10 * C + H + seed + SEED_SHIFT.get(shape, 0))
    x = (rng.standard_normal(shape) * 2).astype(np.float32)
    hi = max(C, 2)
    lab = void_runs(rng.integers(0, hi, (B, H * W)), rng).reshape(B, H, W)
    for a in (x, lab):
        a.setflags(write=False)
    p = lovasz_ref.softmax(x)
    p.setflags(write=False)
    return x, p, lab


@functools.lru_cache(maxsize=None)
def reference(shape, mode, classes, per_image, ignore):
    x, p, lab = inputs(shape)
    src = p if mode == 'probas' else (x[:, :1] if mode == 'hinge' else x)
    cl = classes if isinstance(classes, str) else list(classes)
    gap = lovasz_ref.min_error_gap(src, lab, mode, cl, per_image, ignore)
    return lovasz_ref.lovasz(src, lab, mode, cl, per_image, ignore) + (gap,)


def run(dev, fn, x, scale=SCALE):
    xt = torch.from_numpy(np.array(x)).to(dev).requires_grad_(True)
    loss = fn(xt)
    (loss * float(scale)).backward()
    return float(loss.detach()), xt.grad.cpu().numpy()


def labels_to(dev, lab, u8):
    t = torch.from_numpy(np.array(lab))
    return (t.to(torch.uint8) if u8 else t).to(dev)


def check(tag, loss, grad, ref_loss, ref_grad, scale=SCALE):
    ref_grad = ref_grad * scale
    excess = np.abs(grad - ref_grad) - 1e-4 * np.abs(ref_grad)
    print(f'LOVASZ_ERR {tag} loss_rel={abs(loss - ref_loss) / max(abs(ref_loss), 1e-30):.3e} '
          f'grad_abs={np.abs(grad - ref_grad).max():.3e} grad_abs_minus_rtol={excess.max():.3e}')
    np.testing.assert_allclose(loss, ref_loss, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-4, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------
# 1. against lovasz_ref
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ignore', [None, 255])
@pytest.mark.parametrize('classes', ['present', 'all', 'list'])
@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_softmax_vs_ref(hip_device, shape, per_image, classes, ignore):
    """lovasz_softmax on host-softmaxed probabilities, and the fused softmax on the raw logits.  With ignore=None the
    255 labels stay in the map: they match no class and are background for all.  Labels are uint8 in the per-image
    cases and int64 batch-wide."""
    import losses
    import lovasz
    from ssseg import native as N
    from ssseg import ops
    x, p, lab = inputs(shape)
    cl = tuple(class_list(shape[1])) if classes == 'list' else classes
    arg = list(cl) if classes == 'list' else cl
    lt = labels_to(hip_device, lab, u8=per_image)
    tag = f'{shape} per_image={per_image} classes={classes} ignore={ignore}'

    ref_loss, ref_grad, gap = reference(shape, 'probas', cl, per_image, ignore)
    assert gap > 0, 'two equal valid errors in a segment: change the seed'
    loss, grad = run(hip_device, lambda t: lovasz.lovasz_softmax(t, lt, arg, per_image, ignore), p)
    check('probas ' + tag, loss, grad, ref_loss, ref_grad)

    ref_loss, ref_grad, gap = reference(shape, 'softmax', cl, per_image, ignore)
    assert gap > 0
    fused = losses.LovaszSoftmaxLossWithLogits(arg, per_image, ignore)   # on the label map: void pixels stay void
    loss, grad = run(hip_device, lambda t: fused(t, lt), x)
    check('fused ' + tag, loss, grad, ref_loss, ref_grad)
    ids, present = (list(range(shape[1])), classes == 'present') if classes != 'list' else (arg, False)
    op = run(hip_device, lambda t: ops.lovasz_general(t, lt, N.LOVASZ_SOFTMAX, ids, per_image, ignore, present), x)
    assert op[0] == loss and np.array_equal(op[1], grad)


@pytest.mark.parametrize('classes', ['present', [0, 2]])
@pytest.mark.parametrize('per_image', [False, True])
def test_loss_class_reads_dense_targets(hip_device, per_image, classes):
    """LovaszSoftmaxLossWithLogits takes the argmax of a one-hot or soft target inside the kernels: bitwise the fused
    op on the integer labels."""
    import losses
    from ssseg import native as N
    from ssseg import ops
    shape = (3, 3, 23, 29)
    x, _, lab = inputs(shape)
    lab = lab % 3
    onehot = np.eye(3, dtype=np.float32)[lab].transpose(0, 3, 1, 2)
    soft = onehot * 0.8 + 0.1 / 3
    ids, present = ([0, 1, 2], True) if classes == 'present' else (classes, False)
    lt = labels_to(hip_device, lab, u8=False)
    want = run(hip_device, lambda t: ops.lovasz_general(t, lt, N.LOVASZ_SOFTMAX, ids, per_image, None, present), x)
    fn = losses.LovaszSoftmaxLossWithLogits(classes, per_image)
    for target in (onehot, soft):
        tt = torch.from_numpy(np.ascontiguousarray(target)).to(hip_device)
        got = run(hip_device, lambda t: fn(t, tt), x)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])


def test_flat_functions_are_one_group(hip_device):
    import lovasz
    _, p, lab = inputs((3, 3, 23, 29))
    lab = lab % 3
    lt = labels_to(hip_device, lab, u8=False)
    want = run(hip_device, lambda t: lovasz.lovasz_softmax(t, lt, 'present', False), p)
    got = run(hip_device, lambda t: lovasz.lovasz_softmax_flat(t.permute(0, 2, 3, 1).reshape(-1, 3), lt.reshape(-1)), p)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    x = inputs((3, 1, 23, 29))[0][:, 0]
    ht = labels_to(hip_device, lab % 2, u8=False)
    want = run(hip_device, lambda t: lovasz.lovasz_hinge(t, ht, per_image=False), x)
    got = run(hip_device, lambda t: lovasz.lovasz_hinge_flat(t.reshape(-1), ht.reshape(-1)), x)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    empty = torch.zeros(0, 3, device=hip_device, requires_grad=True)
    assert float(lovasz.lovasz_softmax_flat(empty, torch.zeros(0, dtype=torch.long, device=hip_device)).detach()) == 0


def test_xloss_functions_route_to_the_bce_kernel(hip_device):
    import lovasz
    from ssseg import ops
    x = torch.from_numpy(np.array(inputs((3, 1, 23, 29))[0][:, 0])).to(hip_device)
    t = torch.from_numpy(inputs((3, 3, 23, 29))[2] % 2).to(hip_device)
    want = ops.bce_with_logits_mean(x, t.float())
    assert torch.equal(lovasz.binary_xloss(x, t), want)
    assert torch.equal(lovasz.StableBCELoss()(x, t.float()), want)


# ---------------------------------------------------------------------------------------------------------------
# 2. against the reference fixtures
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', EXPECTED)
def test_vs_reference_golden(hip_device, name):
    """the bounds of golden G4: loss rtol 1e-5, gradient rtol 1e-5 / atol 1e-6"""
    import lovasz
    g = golden(f'lovasz_gen_{name}.npz')
    x, lab, mode, classes, per_image, ignore = fixture_call(g)
    lt = labels_to(hip_device, lab, u8=False)
    if mode == 'hinge':
        fn = lambda t: lovasz.lovasz_hinge(t, lt, per_image, ignore)   # noqa: E731
    else:
        fn = lambda t: lovasz.lovasz_softmax(t, lt, classes, per_image, ignore)   # noqa: E731
    loss, grad = run(hip_device, fn, x, scale=float(g['w']))
    np.testing.assert_allclose(loss, float(g['loss']), rtol=1e-5)
    np.testing.assert_allclose(grad, g['grad'], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------
# 3. exact zeros
# ---------------------------------------------------------------------------------------------------------------
def _zero(t):
    return torch.equal(t, torch.zeros_like(t))


def test_exact_zeros_ignored_unselected_absent(hip_device):
    import lovasz
    from ssseg import native as N
    from ssseg import ops
    shape = (3, 3, 23, 29)
    x, p, lab = inputs(shape)
    lt = labels_to(hip_device, lab, u8=False)
    void = (lt == 255)[:, None].expand(-1, 3, -1, -1)
    for per_image in (False, True):
        pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
        lovasz.lovasz_softmax(pt, lt, 'all', per_image, 255).backward()
        assert _zero(pt.grad[void]) and not _zero(pt.grad[~void])
        xt = torch.from_numpy(np.array(x)).to(hip_device).requires_grad_(True)
        ops.lovasz_general(xt, lt, N.LOVASZ_SOFTMAX, [0, 1, 2], per_image, 255).backward()
        assert _zero(xt.grad[void]) and not _zero(xt.grad[~void])
        # unselected channels
        pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
        lovasz.lovasz_softmax(pt, lt, [1], per_image, 255).backward()
        assert _zero(pt.grad[:, 0]) and _zero(pt.grad[:, 2]) and not _zero(pt.grad[:, 1])
        # a class absent from every group: counted by 'all', exact zeros under 'present'
        l2 = torch.where(lt == 2, torch.zeros_like(lt), lt)
        pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
        lovasz.lovasz_softmax(pt, l2, 'present', per_image, 255).backward()
        assert _zero(pt.grad[:, 2]) and not _zero(pt.grad[:, 1])
        pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
        lovasz.lovasz_softmax(pt, l2, 'all', per_image, 255).backward()
        assert not _zero(pt.grad[:, 2])


def test_all_void_group_and_batch(hip_device):
    import lovasz
    from ssseg import native as N
    from ssseg import ops
    shape = (3, 3, 23, 29)
    x, p, lab = inputs(shape)
    lab = lab.copy()
    lab[1] = 255
    lt = labels_to(hip_device, lab, u8=True)
    # one all-void image: its gradient is zero, and the loss is the mean over three images of which it adds 0
    for classes in ('present', 'all'):
        pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
        loss = lovasz.lovasz_softmax(pt, lt, classes, True, 255)
        loss.backward()
        assert _zero(pt.grad[1]) and not _zero(pt.grad[0]) and not _zero(pt.grad[2])
        two = lovasz.lovasz_softmax(pt.detach()[[0, 2]], lt[[0, 2]], classes, True, 255)
        np.testing.assert_allclose(float(loss), float(two) * 2 / 3, rtol=1e-6)
    ht = labels_to(hip_device, np.where(lab == 255, 255, lab % 2), u8=True)
    xt = torch.from_numpy(np.array(x[:, :1])).to(hip_device).requires_grad_(True)
    lovasz.lovasz_hinge(xt[:, 0], ht, True, 255).backward()
    assert _zero(xt.grad[1]) and not _zero(xt.grad[0])
    # an all-void batch: loss and gradient are exactly zero
    allvoid = torch.full((3, 23, 29), 255, dtype=torch.long, device=hip_device)
    for per_image in (False, True):
        for classes in ('present', 'all', [1, 2]):
            pt = torch.from_numpy(np.array(p)).to(hip_device).requires_grad_(True)
            loss = lovasz.lovasz_softmax(pt, allvoid, classes, per_image, 255)
            loss.backward()
            assert _zero(loss) and _zero(pt.grad)
        xt = torch.from_numpy(np.array(x)).to(hip_device).requires_grad_(True)
        loss = ops.lovasz_general(xt, allvoid, N.LOVASZ_SOFTMAX, [0, 1, 2], per_image, 255, True)
        loss.backward()
        assert _zero(loss) and _zero(xt.grad)
        xt = torch.from_numpy(np.array(x[:, 0])).to(hip_device).requires_grad_(True)
        loss = lovasz.lovasz_hinge(xt, allvoid, per_image, 255)
        loss.backward()
        assert _zero(loss) and _zero(xt.grad)


# ---------------------------------------------------------------------------------------------------------------
# 4. ties
# ---------------------------------------------------------------------------------------------------------------
def _tie_sums(grad, src, lab, mode, classes, per_image, ignore):
    """per (segment, tie group): the sum of the Lovász weights -grad / sign over the pixels of the group"""
    B, C = src.shape[:2]
    flat = grad.reshape(B, C, -1).transpose(1, 0, 2).reshape(C, -1).astype(np.float64)
    xs = src.reshape(B, C, -1).transpose(1, 0, 2).reshape(C, -1)
    out = []
    for g, k, ch, idx, fg, err in lovasz_ref.segments(src.reshape(B, C, -1), lab.reshape(B, -1), mode, classes, per_image,
                                                      ignore):
        sg = -(2 * fg - 1) * (err > 0) if mode == 'hinge' else -np.sign(fg - xs[ch, idx])
        for e in np.unique(err):
            m = (err == e) & (sg != 0)
            if m.any():
                out.append((flat[ch, idx[m]] / sg[m]).sum())
    return np.array(out)


@pytest.mark.parametrize('per_image', [False, True])
def test_ties_loss_and_tie_group_weights(hip_device, per_image):
    """logits x30 saturate the softmax to exact 0 / 1 in most pixels; hinge logits come from a five-value grid.  The
    gradient inside a tie depends on the sort's tie order; the loss and the weight sum of each tie group do not."""
    import lovasz
    shape = (2, 5, 32, 33)
    x, _, lab = inputs(shape)
    p = lovasz_ref.softmax(x * 15)   # the logits are N(0, 1) x 2: x 30 in all
    assert lovasz_ref.min_error_gap(p, lab, 'probas', 'all', per_image, 255) == 0
    lt = labels_to(hip_device, lab, u8=True)
    for classes in ('present', 'all'):
        loss, grad = run(hip_device, lambda t: lovasz.lovasz_softmax(t, lt, classes, per_image, 255), p, 1.0)
        ref_loss, ref_grad = lovasz_ref.lovasz(p, lab, 'probas', classes, per_image, 255)
        np.testing.assert_allclose(loss, ref_loss, rtol=1e-5)
        np.testing.assert_allclose(_tie_sums(grad, p, lab, 'probas', classes, per_image, 255),
                                   _tie_sums(ref_grad, p, lab, 'probas', classes, per_image, 255), rtol=1e-4, atol=1e-5)
    rng = np.random.default_rng(7)
    hx = rng.choice(np.array([-1, 0, 0.5, 1, 2], np.float32), size=(2, 1, 32, 33))
    hl = np.where(lab == 255, 255, lab % 2)
    ht = labels_to(hip_device, hl, u8=True)
    loss, grad = run(hip_device, lambda t: lovasz.lovasz_hinge(t[:, 0], ht, per_image, 255), hx, 1.0)
    ref_loss, ref_grad = lovasz_ref.lovasz(hx, hl, 'hinge', [1], per_image, 255)
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-5)
    np.testing.assert_allclose(_tie_sums(grad, hx, hl, 'hinge', [1], per_image, 255),
                               _tie_sums(ref_grad, hx, hl, 'hinge', [1], per_image, 255), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------
# 5. bitwise
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['probas', 'softmax', 'hinge'])
def test_bwd_from_fwd_repeat_and_retained_graph_bitwise(hip_device, mode):
    """The autograd backward scatters what the forward left in its workspace; ssseg_lovasz_gen_bwd sorts again: the
    same bits, ties included.  A second run and a second backward through a retained graph repeat them."""
    import ctypes
    from ssseg import native as N
    from ssseg import ops
    shape = (2, 5, 32, 33)
    x, _, lab = inputs(shape)
    rng = np.random.default_rng(3)
    if mode == 'hinge':
        src = rng.choice(np.array([-1, 0, 0.5, 1, 2, 0.25], np.float32), size=(2, 1, 32, 33))
        lab, ids, code = np.where(lab == 255, 255, lab % 2), [1], N.LOVASZ_HINGE
    else:
        src = lovasz_ref.softmax(x * 15) if mode == 'probas' else np.round(x * 2) / 2   # ties either way
        ids, code = [0, 1, 2, 3, 4], (N.LOVASZ_PROBAS if mode == 'probas' else N.LOVASZ_SOFTMAX)
    lt = labels_to(hip_device, lab, u8=False)
    B, C = src.shape[:2]
    for per_image in (False, True):
        xt = torch.from_numpy(np.array(src)).to(hip_device).requires_grad_(True)
        loss = ops.lovasz_general(xt, lt, code, ids, per_image, 255, mode != 'hinge')
        (loss * 0.3).backward(retain_graph=True)
        g1 = xt.grad.clone()
        xt.grad = None
        (loss * 0.3).backward()
        assert torch.equal(xt.grad, g1)
        x2 = torch.from_numpy(np.array(src)).to(hip_device).requires_grad_(True)
        loss2 = ops.lovasz_general(x2, lt, code, ids, per_image, 255, mode != 'hinge')
        (loss2 * 0.3).backward()
        assert torch.equal(loss2, loss) and torch.equal(x2.grad, g1)
        gx = torch.empty_like(g1)
        go = torch.full((), 0.3, device=hip_device)
        nb = N.lib().ssseg_lovasz_gen_workspace_bytes(B, C, 32 * 33, int(per_image), len(ids))
        ws = N.workspace(nb, hip_device)
        N.call('ssseg_lovasz_gen_bwd', N.dev_ptr(xt.detach()), N.dev_ptr(lt), N.LOVASZ_LABEL_I64, B, C, 32 * 33, code,
               int(per_image), int(mode != 'hinge'), (ctypes.c_int64 * len(ids))(*ids), len(ids), 1, 255,
               N.dev_ptr(go), N.dev_ptr(gx), N.dev_ptr(ws), nb, N.stream())
        torch.cuda.synchronize()
        assert torch.equal(gx, g1)


# ---------------------------------------------------------------------------------------------------------------
# 6. hinge
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ignore', [None, 255])
@pytest.mark.parametrize('per_image', [False, True])
@pytest.mark.parametrize('shape', HINGE_SHAPES)
def test_hinge_vs_ref(hip_device, shape, per_image, ignore):
    import losses
    import lovasz
    x, _, lab = inputs(shape)
    if ignore is None:
        lab = lab % 2    # without a void label the map is 0 / 1 (255 -> 1)
    ref_loss, ref_grad = lovasz_ref.lovasz(x, lab, 'hinge', [1], per_image, ignore)
    assert lovasz_ref.min_error_gap(x, lab, 'hinge', [1], per_image, ignore) > 0
    lt = labels_to(hip_device, lab, u8=per_image)
    loss, grad = run(hip_device, lambda t: lovasz.lovasz_hinge(t[:, 0], lt, per_image, ignore), x)
    check(f'hinge {shape} per_image={per_image} ignore={ignore}', loss, grad, ref_loss, ref_grad)
    # the config-level class on a float mask of the logits' shape: the same kernels, the same bits
    mask = torch.from_numpy(lab.astype(np.float32)[:, None]).to(hip_device)
    got = run(hip_device, lambda t: losses.LovaszHingeLossWithLogits(per_image, ignore)(t, mask), x)
    assert got[0] == loss and np.array_equal(got[1], grad)


@pytest.mark.parametrize('per_image', [False, True])
def test_hinge_all_errors_negative(hip_device, per_image):
    """every pixel classified with a margin above 1: relu cuts every error, the loss is 0 and so is the gradient"""
    import lovasz
    _, _, lab = inputs((3, 1, 23, 29))
    lab = lab % 2
    x = ((2.0 * lab - 1.0) * (1.5 + np.arange(lab.size).reshape(lab.shape) % 7)).astype(np.float32)
    xt = torch.from_numpy(np.array(x)).to(hip_device).requires_grad_(True)
    loss = lovasz.lovasz_hinge(xt, labels_to(hip_device, lab, u8=False), per_image)
    loss.backward()
    assert _zero(loss) and _zero(xt.grad)


# ---------------------------------------------------------------------------------------------------------------
# 7. captured replay
# ---------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_with_new_logits_and_labels(hip_device):
    """Forward and backward of LovaszSoftmaxLossWithLogits('present') next to a dense CE inside CalculateLoss, captured
    once and replayed: with new logits, and with a label map from which a class present at capture time is gone.  The
    'present' decision is taken on the device, so every replay equals the eager result bit for bit."""
    import losses
    from ssseg.graph import StepGraph
    shape = (2, 5, 32, 33)
    x0, _, lab = inputs(shape)
    x1 = inputs(shape, seed=1)[0]
    lab0 = lab % 5
    lab2 = np.where(lab0 == 3, 0, lab0)
    assert (lab0 == 3).any()
    eye = np.eye(5, dtype=np.float32)
    t0, t2 = (torch.from_numpy(np.ascontiguousarray(eye[v].transpose(0, 3, 1, 2))).to(hip_device) for v in (lab0, lab2))
    x0, x1 = (torch.from_numpy(np.array(v)).to(hip_device) for v in (x0, x1))
    calc = losses.CalculateLoss([{'loss_fn': losses.LovaszSoftmaxLossWithLogits('present', False, 255), 'weight': [1.0]},
                                 {'loss_fn': losses.DenseCrossEntropyLossWithLogits('mean'), 'weight': [0.5]}])

    def step(x, t):
        xr = x.detach().requires_grad_(True)
        loss = calc([xr], t)
        return loss, torch.autograd.grad(loss, xr)[0]

    eager = [tuple(v.clone() for v in step(x, t)) for x, t in ((x0, t0), (x1, t0), (x1, t2))]
    assert not torch.equal(eager[1][0], eager[2][0])
    graph = StepGraph(step, x0, t0)
    for (x, t), want in zip(((x0, t0), (x1, t0), (x1, t2)), eager):
        loss, grad = graph(x, t)
        torch.cuda.synchronize()
        assert torch.equal(loss, want[0]) and torch.equal(grad, want[1])


# ---------------------------------------------------------------------------------------------------------------
# 8. the binary call keeps its path
# ---------------------------------------------------------------------------------------------------------------
def test_binary_per_image_call_unchanged(hip_device):
    """lovasz_softmax(x, labels, classes=[1], per_image=True) on two-channel input is ops.lovasz_binary without the
    valid-sample weighting, bit for bit; where every image has foreground, binary_lovasz_loss_with_logits' weighted
    form is the same mean up to its 0.001 in the denominator."""
    import losses
    import lovasz
    from ssseg import ops
    rng = np.random.default_rng(11)
    B, H, W = 3, 70, 66
    x = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    lab = (rng.random((B, H, W)) > 0.6).astype(np.int64)
    lt = torch.from_numpy(lab).to(hip_device)
    target = torch.stack([lt == 0, lt == 1], 1).float()
    got = run(hip_device, lambda t: lovasz.lovasz_softmax(t, lt, classes=[1], per_image=True), x)
    want = run(hip_device, lambda t: ops.lovasz_binary(t, target, valid_weighted=False), x)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    ref_loss, ref_grad = lovasz_ref.lovasz(x, lab, 'probas', [1], True, None)
    assert lovasz_ref.min_error_gap(x, lab, 'probas', [1], True, None) > 0
    check('binary per-image', got[0], got[1], ref_loss, ref_grad)
    weighted = run(hip_device, lambda t: losses.binary_lovasz_loss_with_logits(t, target), x)
    np.testing.assert_allclose(weighted[0] * (B + 0.001) / B, got[0], rtol=1e-6)
    np.testing.assert_allclose(weighted[1] * np.float32((B + 0.001) / B), got[1], rtol=1e-5, atol=1e-8)
