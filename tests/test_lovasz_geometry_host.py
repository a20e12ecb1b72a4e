"""Host-side proof (no GPU) of the designs in exact_lovasz.py that test_lovasz_geometry.py runs on the device.

For every case:
  1. the design is exact: the fp32 error |fg - x| (hinge: 1 - x * sign) of every valid pixel equals the designed
     multiple of 2^-24 (2^-22) bit for bit, the errors of a segment are distinct, and the designed ranks are the stable
     descending argsort (the 2^24-pixel case skips the argsort);
  2. the expectation built from the ranks equals lovasz_ref.lovasz (oracle.losses_ref.binary_lovasz for the binary
     entry points) bit for bit, loss and gradient;
  3. at least half of the adjacent sorted positions hold weights that differ bitwise, so a pixel moved to a
     neighbouring rank changes the gradient;
  4. the shape stands on the intended side of the launch threshold it is there for (exact_lovasz.CROSSES, thresholds
     named as in csrc/lovasz.hip);
  5. the fp32 CPU restatement of the gradient, computed operation by operation as the kernels do, meets the device
     bound itself.
The fused-softmax probe cases: one-hot background in fp32, 16 probes whose fp64 errors are 1e-3 apart in every class.
"""
import numpy as np
import pytest

import exact_lovasz as E
import lovasz_ref
from oracle import losses_ref

F32, F64 = np.float32, np.float64


def check_design(spec, argsort=True):
    d = E.build(spec)
    x, lab = d.x.reshape(spec.B, spec.C, spec.HW), d.lab.reshape(spec.B, spec.HW)
    nseg = 0
    for g, k, ch, idx, fg, err in lovasz_ref.segments(x, lab, spec.mode, spec.classes_arg, spec.per_image, spec.ignore):
        n = idx.size
        if n == 0:
            continue
        r = d.rank[ch, idx]
        assert err.dtype == F32 and r.min() == 0 and r.max() == n - 1
        want = E.design_errors(spec, n, r)
        assert np.array_equal(err.astype(F64), want)                         # |fg - x| == e, bit for bit
        if spec.mode == 'hinge':
            assert (want > 0).any() and (want < 0).any() and (want == 0).sum() == 1
        else:
            assert want.min() > 0 and want.max() <= 1
        if argsort:
            assert np.array_equal(np.argsort(-err, kind='stable'), np.argsort(r))   # distinct, and ranked as designed
        else:
            assert np.array_equal(np.bincount(r, minlength=n), np.ones(n, np.int64))   # a permutation: distinct errors
        nseg += 1
    return nseg


@pytest.mark.parametrize('name', [s.name for s in E.GENERAL])
def test_general_design(name):
    spec = E.BY_NAME[name]
    assert E.CROSSES[name](spec)                                             # 4
    nseg = check_design(spec)                                                # 1
    exp = E.expected(spec)
    assert nseg == exp.nseg
    d = E.build(spec)
    loss, grad = lovasz_ref.lovasz(d.x, d.lab, spec.mode, spec.classes_arg, spec.per_image, spec.ignore)   # 2
    assert loss == exp.loss and loss.dtype == F32
    assert np.array_equal(grad, exp.grad.astype(F32))
    print(f'{name}: loss {float(loss):.9g} segments {exp.nseg} diversity {exp.diversity:.3f} exact {exp.exact}')
    if spec.void != 'last:1':                                                # one valid pixel: no adjacent positions
        assert exp.diversity >= 0.5                                          # 3
    worst = E.check_grad(exp.grad32, exp.grad * float(E.UPSTREAM), exp.exact)   # 5
    print(f'{name}: fp32 restatement within {worst:.3f} x 2^-24 |ref|')
    assert np.abs(exp.grad).max() > 0


def test_void_cases_ignore_what_they_should():
    for name, nvalid in (('void_131072', 131072), ('void_131073', 131073), ('void_one', 1)):
        spec = E.BY_NAME[name]
        lab = E.build(spec).lab.reshape(-1)
        assert int((lab != 255).sum()) == nvalid
        tiles_void = (lab == 255)[:E.tiles(spec.HW) * E.TILE - E.TILE].reshape(-1, E.TILE).all(1)
        assert tiles_void.sum() >= 60                                        # whole void tiles
        if name == 'void_one':
            assert lab[-1] != 255
        else:
            edge = (lab == 255).reshape(-1)[100 * E.TILE - 1:100 * E.TILE + 1]
            assert edge.all()                                                # a void run across a tile edge
        grad = E.expected(spec).grad.reshape(-1)
        assert np.all(grad[lab == 255] == 0) and np.abs(grad[lab != 255]).max() > 0


def test_absent_classes_are_absent():
    for name in ('chunk2_present', 'chunk1_present', 'chunk7_present'):
        spec = E.BY_NAME[name]
        b, c = spec.absent
        lab = E.build(spec).lab
        assert not (lab[b] == c).any() and all((lab[i] == c).any() for i in range(spec.B) if i != b)
        grad = E.expected(spec).grad
        assert np.all(grad[b, c] == 0) and np.abs(grad[b, (c + 1) % spec.C]).max() > 0


def test_length_bound_design():
    """2^24 pixels: the permutation check stands in for the argsort; lovasz_ref.lovasz is not run"""
    spec = E.LENGTH_BOUND
    assert E.CROSSES[spec.name](spec) and check_design(spec, argsort=False) == 1
    exp = E.expected(spec)
    print(f'{spec.name}: loss {float(exp.loss):.9g} diversity {exp.diversity:.3f}')
    assert exp.diversity >= 0.5 and exp.exact
    E.check_grad(exp.grad32, exp.grad * float(E.UPSTREAM), True)


@pytest.mark.parametrize('name', [s.name for s in E.BINARY])
def test_binary_design(name):
    spec = E.BY_NAME[name]
    assert E.CROSSES[name](spec) and spec.C == 2 and spec.per_image
    d = E.build(spec)
    x, lab = d.x.reshape(spec.B, 2, spec.HW), d.lab.reshape(spec.B, spec.HW)
    for b in range(spec.B):
        fg = (lab[b] == 1).astype(F32)
        err = np.abs(fg - x[b, 1])
        r = d.rank[1, b * spec.HW:(b + 1) * spec.HW]
        assert np.array_equal(err.astype(F64), E.design_errors(spec, spec.HW, r))
        assert np.array_equal(np.argsort(-err, kind='stable'), np.argsort(r))
    if spec.nofg is not None:
        assert not lab[spec.nofg].any() and all(lab[b].any() for b in range(spec.B) if b != spec.nofg)
    exp = E.expected_binary(spec)
    loss, grad = losses_ref.binary_lovasz(d.x, E.onehot(spec))
    assert loss == exp.loss
    # binary_lovasz rounds its gradient in fp32 on the way: the fp64 form is held to the device bound against it
    worst_ref = E.check_grad(grad, exp.grad, False)
    worst = E.check_grad(exp.grad32, exp.grad * float(E.UPSTREAM), False)
    print(f'{name}: loss {float(loss):.9g} diversity {exp.diversity:.3f}; binary_lovasz {worst_ref:.3f}, fp32 '
          f'restatement {worst:.3f} x 2^-24 |ref|')
    assert exp.diversity >= 0.5
    assert np.all(exp.grad[:, 0] == 0)


@pytest.mark.parametrize('name', list(E.SOFTMAX_PROBES))
def test_softmax_probe_design(name):
    case = E.softmax_probe_case(name)
    spec = case.spec
    N = spec.B * spec.HW
    assert len(case.sites) == 16 and len(set(case.sites)) == 16
    want = {0, 255, 256, E.TILE - 1, E.TILE, E.GRID_SPAN - 1, E.GRID_SPAN, N - 1}
    for b in range(1, spec.B):
        want |= {b * spec.HW - 1, b * spec.HW}
    assert want <= set(case.sites) and N > E.GRID_SPAN
    assert E.chunk_classes(N, spec.C) < spec.C or spec.B > 1     # a chunk boundary (pixels N - 1 | 0), or images'
    p64 = np.exp(case.x.astype(F64) - case.x.max(1, keepdims=True))
    p64 /= p64.sum(1, keepdims=True)
    p64 = E.planes(p64, spec)
    lab = case.lab.reshape(-1)
    p32 = E.planes(lovasz_ref.softmax(case.x), spec)
    rest = np.ones(N, bool)
    rest[list(case.sites)] = False
    for c in range(spec.C):
        fg = (lab == c).astype(F64)
        assert np.all(np.abs(fg - p32[c])[rest] == 0)                        # one-hot in fp32: error exactly 0
        err = np.sort(np.abs(fg - p64[c])[list(case.sites)])
        assert err[0] >= 1e-3 and np.diff(err).min() >= 1e-3                 # 1e-3 apart, and from the background's 0
    loss, grad = E.softmax_probe_expected(name)
    assert loss > 0 and np.all(E.planes(grad, spec)[:, rest] == 0)
    assert np.all(np.abs(E.planes(grad, spec)[:, list(case.sites)]).max(0) > 0)    # every probe has a gradient
    up = E.probe_upstream(grad)
    assert 2.0 ** -8 <= float(np.abs(grad).max()) * up < 2.0 ** -7 and float(np.log2(up)).is_integer()


def test_bounds_reject_on_the_host():
    """ssseg_lovasz_gen_workspace_bytes is 0 outside L <= 2^24 and G * K <= 65,535 (no device is touched)"""
    from ssseg import native as N
    lib = N.lib()
    assert lib.ssseg_lovasz_gen_workspace_bytes(1, 1, E.MAX_L, 0, 1) > 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1, 1, E.MAX_L + 1, 0, 1) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1, 1, E.MAX_L + 1, 1, 1) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(2, 1, E.MAX_L // 2 + 1, 0, 1) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1285, 51, 2, 1, 51) > 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1286, 51, 2, 1, 51) == 0
    assert lib.ssseg_lovasz_gen_workspace_bytes(1286, 51, 2, 0, 51) > 0      # one group: 51 segments
    assert lib.ssseg_lovasz_sort_workspace_bytes(E.MAX_S, 3) > 0
    assert lib.ssseg_lovasz_sort_workspace_bytes(1, E.MAX_L) > 0
    assert lib.ssseg_lovasz_sort_workspace_bytes(E.MAX_S + 1, 3) == 0
    assert lib.ssseg_lovasz_sort_workspace_bytes(1, E.MAX_L + 1) == 0
    # the 2^24-pixel case: about 340 MB
    nb = lib.ssseg_lovasz_gen_workspace_bytes(1, 1, E.MAX_L, 0, 1)
    assert 320e6 < nb < 360e6
