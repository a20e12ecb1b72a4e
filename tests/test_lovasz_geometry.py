"""GPU tests of the Lovász kernels (csrc/lovasz.hip) at their full-size launch edges, on the designed-rank inputs of
tests/exact_lovasz.py (tests/test_lovasz_geometry_host.py proves the designs and the expectations on the CPU).

The sorted position of every pixel is known by design, so every case compares
  - the loss with the restatement's fp32 value: equal,
  - the gradient at every element, without an absolute term: exactly 0 where the reference is 0; equal to the
    reference where (classes counted) * G and the upstream gradient are powers of two; else within
    K_ROUND * 2^-24 * |ref| of the fp64 reference (exact_lovasz.K_ROUND = 3 fp32 roundings, counted from the source).
The fused-softmax cases follow the probe principle: exact zeros on a one-hot background, 16 probes held to the bounds
of tests/test_lovasz_general.py."""
import ctypes

import numpy as np
import pytest
import torch

import exact_lovasz as E
import lovasz_ref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
UP = float(E.UPSTREAM)
LOSS_TOL = dict(rtol=2e-5, atol=1e-7)     # tests/test_lovasz_general.py check()
GRAD_TOL = dict(rtol=1e-4, atol=2e-6)


def _labels(dev, spec, lab, kind):
    if kind == 'dense':
        return torch.from_numpy(E.onehot(spec)).to(dev)
    t = torch.from_numpy(np.array(lab))
    return {'i64': t, 'u8': t.to(torch.uint8), 'f32': t.to(torch.float32)}[kind].to(dev)


def run_general(dev, spec, x, lab, kind='i64', upstream=UP):
    """(loss fp32, gradient) of forward + backward: lovasz.py's functions on integer labels, ops.lovasz_general on
    float labels and dense targets"""
    import lovasz
    from ssseg import native as N
    from ssseg import ops
    xt = torch.from_numpy(np.array(x)).to(dev).requires_grad_(True)
    lt = _labels(dev, spec, lab, kind)
    ids, present = lovasz_ref.class_ids(spec.classes_arg, spec.C)
    if kind in ('f32', 'dense') or spec.mode == 'softmax':
        code = {'probas': N.LOVASZ_PROBAS, 'softmax': N.LOVASZ_SOFTMAX, 'hinge': N.LOVASZ_HINGE}[spec.mode]
        loss = ops.lovasz_general(xt, lt, code, ids, spec.per_image, spec.ignore, present, dense_target=kind == 'dense')
    elif spec.mode == 'hinge':
        loss = lovasz.lovasz_hinge(xt[:, 0], lt, spec.per_image, spec.ignore)
    else:
        loss = lovasz.lovasz_softmax(xt, lt, spec.classes_arg, spec.per_image, spec.ignore)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return F32(loss.detach().cpu().numpy()), xt.grad.cpu().numpy()


def check_designed(dev, spec, kind='i64'):
    d, exp = E.build(spec), E.expected(spec)
    loss, grad = run_general(dev, spec, d.x, d.lab, kind)
    worst = np.abs(grad.astype(F64) - exp.grad * UP)
    nz = exp.grad != 0
    worst = float((worst[nz] / (E.ULP * np.abs(exp.grad[nz] * UP))).max()) if nz.any() else 0.0
    print(f'LOVASZ_GEO {spec.name} labels={kind} loss {float(loss):.9g} ref {float(exp.loss):.9g} '
          f'rel {abs(float(loss) - float(exp.loss)) / float(exp.loss):.2e}; grad worst {worst:.3f} x 2^-24 |ref| '
          f'(exact asked: {exp.exact})')
    assert loss == exp.loss
    E.check_grad(grad, exp.grad * UP, exp.exact)
    return loss, grad


KINDS = {'grid_one': ('i64', 'u8', 'f32'), 'grid_img': ('i64', 'u8', 'f32', 'dense'), 'void_131073': ('i64', 'u8')}


@pytest.mark.parametrize('name,kind', [(s.name, k) for s in E.GENERAL for k in KINDS.get(s.name, ('i64',))])
def test_designed_ranks(hip_device, name, kind):
    """tile rounds, void pixels at depth, grid strides, chunks by size, many groups (exact_lovasz.GENERAL)"""
    check_designed(hip_device, E.BY_NAME[name], kind)


def test_length_bound(hip_device):
    """L = 2^24, the largest segment: about 340 MB of workspace; the one slow case of this file"""
    check_designed(hip_device, E.LENGTH_BOUND)


def test_out_of_bounds_raise(hip_device):
    import lovasz
    x = torch.zeros(1286, 51, 1, 2, device=hip_device)
    lab = torch.zeros(1286, 1, 2, dtype=torch.uint8, device=hip_device)
    with pytest.raises(ValueError, match='bounds'):
        lovasz.lovasz_softmax(x, lab, 'all', per_image=True)
    assert float(lovasz.lovasz_softmax(x[:1285], lab[:1285], 'all', per_image=True)) > 0
    x = torch.zeros(1, 1, 1, E.MAX_L + 1, device=hip_device)
    lab = torch.zeros(1, 1, E.MAX_L + 1, dtype=torch.uint8, device=hip_device)
    with pytest.raises(ValueError, match='bounds'):
        lovasz.lovasz_softmax(x, lab, [1])
    with pytest.raises(ValueError, match='bounds'):
        lovasz.lovasz_hinge(x[:, 0], lab)


@pytest.mark.parametrize('name', list(E.SOFTMAX_PROBES))
def test_fused_softmax_probes(hip_device, name):
    case = E.softmax_probe_case(name)
    spec = case.spec
    ref_loss, ref_grad = E.softmax_probe_expected(name)
    up = E.probe_upstream(ref_grad)
    loss, grad = run_general(hip_device, spec, case.x, case.lab, upstream=up)
    sites = list(case.sites)
    g, r = E.planes(grad, spec), E.planes(ref_grad, spec).astype(F64) * up
    print(f'LOVASZ_GEO {name} loss {float(loss):.9g} ref {float(ref_loss):.9g}; upstream 2^{int(np.log2(up))}; probes '
          f'grad_abs {np.abs(g[:, sites] - r[:, sites]).max():.3e} of max {np.abs(r).max():.3e}')
    np.testing.assert_allclose(loss, ref_loss, **LOSS_TOL)
    np.testing.assert_allclose(g[:, sites], r[:, sites], **GRAD_TOL)
    rest = np.ones(g.shape[1], bool)
    rest[sites] = False
    assert np.all(g[:, rest] == 0), 'a gradient on the one-hot background'
    assert np.all(np.abs(g[:, sites]).max(0) > 0)


# ---- the binary entry points -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [s.name for s in E.BINARY])
def test_binary_entry_points(hip_device, name):
    """losses.binary_lovasz_loss_with_logits on designed ranks of channel 1: lovasz_prep_kernel / lovasz_grad_kernel /
    lovasz_final_kernel / lovasz_bwd_kernel past the tile rounds, the grid stride and 16 images"""
    import losses
    from ssseg import native as N
    spec = E.BY_NAME[name]
    d, exp = E.build(spec), E.expected_binary(spec)
    xt = torch.from_numpy(np.array(d.x)).to(hip_device).requires_grad_(True)
    tt = torch.from_numpy(E.onehot(spec)).to(hip_device)
    loss = losses.binary_lovasz_loss_with_logits(xt, tt)
    (loss * UP).backward()
    torch.cuda.synchronize()
    got, grad = F32(loss.detach().cpu().numpy()), xt.grad.cpu().numpy()
    print(f'LOVASZ_GEO {name} loss {float(got):.9g} ref {float(exp.loss):.9g}')
    assert got == exp.loss
    worst = E.check_grad(grad, exp.grad * UP, False)
    print(f'LOVASZ_GEO {name} grad worst {worst:.3f} x 2^-24 |ref|')
    assert torch.equal(xt.grad[:, 0], torch.zeros_like(xt.grad[:, 0]))
    if spec.nofg is not None:
        assert torch.equal(xt.grad[spec.nofg], torch.zeros_like(xt.grad[spec.nofg]))
    if name == 'bin_rounds':    # the backward that sorts again: the same bits as the scatter of the forward's workspace
        B, C, HW = spec.B, 2, spec.HW
        gx = torch.empty_like(xt.grad)
        go = torch.full((), UP, device=hip_device)
        nb = N.lib().ssseg_lovasz_workspace_bytes(B, HW)
        ws = N.workspace(nb, hip_device)
        N.call('ssseg_lovasz_bwd', N.dev_ptr(xt.detach()), N.dev_ptr(tt), B, C, HW, N.dev_ptr(go), N.dev_ptr(gx),
               N.dev_ptr(ws), nb, N.stream())
        torch.cuda.synchronize()
        assert torch.equal(gx, xt.grad)


def test_general_bwd_resort_bitwise_at_depth(hip_device):
    """ssseg_lovasz_gen_bwd (sorts again) against the autograd backward (scatters the forward's workspace) at
    T = 65 and G = 2: the same bits"""
    from ssseg import native as N
    spec = E.BY_NAME['rounds_img']
    d = E.build(spec)
    _, grad = run_general(hip_device, spec, d.x, d.lab)
    xt = torch.from_numpy(np.array(d.x)).to(hip_device)
    lt = torch.from_numpy(np.array(d.lab)).to(hip_device)
    gx = torch.empty_like(xt)
    go = torch.full((), UP, device=hip_device)
    nb = N.lib().ssseg_lovasz_gen_workspace_bytes(spec.B, spec.C, spec.HW, 1, 1)
    ws = N.workspace(nb, hip_device)
    N.call('ssseg_lovasz_gen_bwd', N.dev_ptr(xt), N.dev_ptr(lt), N.LOVASZ_LABEL_I64, spec.B, spec.C, spec.HW,
           N.LOVASZ_PROBAS, 1, 0, (ctypes.c_int64 * 1)(1), 1, 0, 0, N.dev_ptr(go), N.dev_ptr(gx), N.dev_ptr(ws), nb,
           N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(gx.cpu().numpy(), grad)
