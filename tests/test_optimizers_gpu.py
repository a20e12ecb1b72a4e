"""The fused device optimizers (csrc/optim.hip: ssseg.optim.Adam and the `optimizers` package) on the GPU.

Yardstick: tests/optim_ref.py run in fp64.  The device result has to be as close to it as the reference classes' own
fp32 run is, per tensor and per stored step, for the parameters and every state tensor:

    e_dev = max|device - fp64|,  e_ref = max|reference fp32 - fp64|,  e_dev <= 4 * e_ref + 2 ulp_fp32(max|tensor|)

(4: the project's margin for "as good as the reference's own fp32", covering expf / fp64-pow implementation
differences; the ulp floor covers tensors where the reference happens to be exact.)  `ratio` below is
e_dev / (4 * e_ref + 2 ulp); the worst ratios measured per mode are recorded in DESIGN.md §10.
"""
import functools
import json

import numpy as np
import pytest
import torch

from conftest import golden
from optim_ref import RefOptim, replay

pytestmark = pytest.mark.gpu

CASES = ('ranger', 'adamod', 'diffgrad_v0', 'diffgrad_v2', 'diffmod', 'adam')


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(golden arrays, meta, fp64 restatement at the stored steps): computed once, shared, never modified."""
    z = golden(f'optim_{case}.npz')
    meta = json.loads(str(z['meta']))
    ref64, _ = replay(z, meta, torch.float64)
    return z, meta, ref64


def ratio(dev, ref32, ref64):
    """e_dev / (4 e_ref + 2 ulp_fp32(max|tensor|)); <= 1 passes."""
    dev, ref32, ref64 = (t.detach().cpu().double().reshape(-1) for t in (dev, ref32, ref64))
    e_dev = (dev - ref64).abs().max().item()
    e_ref = (ref32 - ref64).abs().max().item()
    ulp = float(np.spacing(np.float32(ref64.abs().max().item())))
    if not np.isfinite(e_dev):
        return float('inf')
    return e_dev / (4 * e_ref + 2 * ulp)


def make_opt(algo, params, ctor):
    import optimizers
    from ssseg import optim
    cls = {'ranger': optimizers.Ranger, 'adamod': optimizers.AdaMod, 'diffgrad': optimizers.DiffGrad,
           'diffmod': optimizers.DiffMod, 'adam': optim.Adam}[algo]
    return cls(params, **ctor)


class Device:
    """A module whose parameters are the given flat tensors, on a flat arena, with its fused optimizer."""

    def __init__(self, algo, tensors, ctor, device):
        from ssseg import arena
        self.mod = torch.nn.Module()
        self.mod.ps = torch.nn.ParameterList([torch.nn.Parameter(t.detach().clone().float()) for t in tensors])
        self.mod.to(device)
        self.arena = arena.attach(self.mod)
        self.params = list(self.mod.ps)
        self.opt = make_opt(algo, self.params, ctor)
        self.keys = tuple(self.opt.STATE_KEYS)

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad.copy_(torch.as_tensor(g).to(p.device, torch.float32).view_as(p))

    def flat_grads(self, grads):
        """The gradients laid out like the gradient arena (padding zero), on the device."""
        flat = torch.zeros_like(self.arena.grad)
        for p, g in zip(self.params, grads):
            o, n = self.arena.slot(p)
            flat[o:o + n] = torch.as_tensor(g).to(flat.device, torch.float32).reshape(-1)
        return flat

    def step(self, grads, **kw):
        self.set_grads(grads)
        self.opt.step(**kw)

    def tensors(self):
        """{(key, i): cpu clone} of the parameters ('p') and every state tensor."""
        out = {}
        for i, p in enumerate(self.params):
            out['p', i] = p.detach().cpu().clone()
            for k in self.keys:
                out[k, i] = self.opt.state[p][k].detach().cpu().clone()
        return out

    def padding_is_clean(self):
        used = torch.zeros(self.arena.numel, dtype=torch.bool)
        for p in self.params:
            o, n = self.arena.slot(p)
            used[o:o + n] = True
        pad = self.arena.data.detach().cpu()[~used]
        return bool((pad == 0).all())


def golden_grads(z, meta, t):
    return [z[f'grad_{t}_{i}'] for i in range(len(meta['sizes']))]


def run_golden(case, device, mutate=None, first=1, dev=None):
    """Replay the recorded gradients through the device optimizer; the worst ratio over tensors and stored steps."""
    z, meta, ref64 = case_data(case)
    n = len(meta['sizes'])
    if dev is None:
        dev = Device(meta['algo'], [torch.from_numpy(z[f'init_{i}']) for i in range(n)], meta['ctor'], device)
    worst, where = 0.0, None
    for t in range(first, meta['T'] + 1):
        if mutate is not None:
            mutate(dev, t)
        dev.step(golden_grads(z, meta, t))
        if t in meta['steps']:
            for (k, i), v in dev.tensors().items():
                r = ratio(v, torch.from_numpy(z[f'{k}_{t}_{i}']), ref64[k, t, i])
                if r > worst:
                    worst, where = r, (k, t, i)
    assert dev.padding_is_clean()
    return worst, where, dev


# ---- 1. parity with the reference's recorded runs, every mode ----
@pytest.mark.parametrize('case', CASES)
def test_parity_with_reference_golden(hip_device, case):
    worst, where, dev = run_golden(case, hip_device)
    print(f'optim parity {case}: worst ratio {worst:.4f} at (key, step, tensor) {where}')
    assert worst <= 1.0, (worst, where)
    assert dev.opt.step_count() == 12


def test_parity_check_detects_mutations(hip_device):
    """The bound is not vacuous: a previous_grad that is not carried between steps, and a Lookahead that is never
    applied, both fail it."""
    def drop_previous_grad(dev, t):
        dev.opt.bufs['previous_grad'].zero_()
    worst, where, _ = run_golden('diffmod', hip_device, mutate=drop_previous_grad)
    assert worst > 1.0, (worst, where)

    def never_lookahead(dev, t):
        dev.opt.param_groups[0]['k'] = 10 ** 6
    worst, where, _ = run_golden('ranger', hip_device, mutate=never_lookahead)
    assert worst > 1.0, (worst, where)


# ---- 2. more than one grid sweep ----
@pytest.mark.parametrize('algo,ctor,hyper', [
    ('diffmod', dict(lr=1e-2, weight_decay=1e-2, len_memory=10), dict(lr=1e-2, weight_decay=1e-2, beta3=1 - (1 / 10))),
    ('ranger', dict(lr=1e-2, weight_decay=1e-2, k=2), dict(lr=1e-2, weight_decay=1e-2, k=2)),
])
def test_more_than_one_grid_sweep(hip_device, algo, ctor, hyper):
    n = 2 * 2 ** 20 + 1027          # past 256*8 blocks x 256 threads x 4, ragged tail
    g = torch.Generator().manual_seed(7)
    init = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(2)]
    dev = Device(algo, [init], ctor, hip_device)
    r32 = RefOptim(algo, [init], dtype=torch.float32, **hyper)
    r64 = RefOptim(algo, [init], dtype=torch.float64, **hyper)
    for gr in grads:
        dev.step([gr])
        r32.step([gr])
        r64.step([gr])
    got = dev.tensors()
    for k in ('p',) + dev.keys:
        a32, a64 = (r.params[0] if k == 'p' else r.state[0][k] for r in (r32, r64))
        r = ratio(got[k, 0], a32, a64)
        assert r <= 1.0, (k, r)
    assert dev.padding_is_clean()


# ---- 3. clip ----
@pytest.mark.parametrize('algo,ctor,hyper', [
    ('adamod', dict(lr=1e-2, weight_decay=1e-2), dict(lr=1e-2, weight_decay=1e-2)),
    ('ranger', dict(lr=1e-2, weight_decay=1e-2, k=2), dict(lr=1e-2, weight_decay=1e-2, k=2)),
    ('adam', dict(lr=1e-2, weight_decay=1e-2), dict(lr=1e-2, weight_decay=1e-2)),
])
@pytest.mark.parametrize('rel', (2.0, 0.25))     # max_norm above / below the gradient norm
def test_clip(hip_device, algo, ctor, hyper, rel):
    z, meta, _ = case_data('adamod')
    n = len(meta['sizes'])
    init = [torch.from_numpy(z[f'init_{i}']) for i in range(n)]
    steps = [[torch.from_numpy(g) for g in golden_grads(z, meta, t)] for t in (1, 2)]
    dev = Device(algo, init, ctor, hip_device)
    refs = {dt: RefOptim(algo, init, dtype=dt, **hyper) for dt in (torch.float32, torch.float64)}
    for grads in steps:
        max_norm = rel * torch.cat([g.reshape(-1) for g in grads]).norm().item()
        dev.step(grads, max_norm=max_norm)
        for dt, r in refs.items():
            gs = [torch.nn.Parameter(torch.zeros_like(g, dtype=dt)) for g in grads]
            for q, g in zip(gs, grads):
                q.grad = g.clone().to(dt)
            total = torch.nn.utils.clip_grad_norm_(gs, max_norm)
            assert (total.item() > max_norm) == (rel < 1)
            r.step([q.grad for q in gs])
    got = dev.tensors()
    for i in range(n):
        for k in ('p',) + dev.keys:
            a32, a64 = (r.params[i] if k == 'p' else r.state[i][k] for r in (refs[torch.float32], refs[torch.float64]))
            r = ratio(got[k, i], a32, a64)
            assert r <= 1.0, (k, i, r)


# ---- 4. loss-scale skip ----
@pytest.mark.parametrize('case', ('diffmod', 'ranger', 'adam'))
def test_loss_scale_skip(hip_device, case):
    from ssseg import amp
    z, meta, _ = case_data(case)
    n = len(meta['sizes'])
    init = [torch.from_numpy(z[f'init_{i}']) for i in range(n)]
    dev = Device(meta['algo'], init, meta['ctor'], hip_device)
    twin = Device(meta['algo'], init, meta['ctor'], hip_device)      # no scaler, raw gradients
    dev.opt.grad_scaler = amp.GradScaler(hip_device)
    before = dev.tensors()
    arenas = {k: b.clone() for k, b in dev.opt.bufs.items()}
    grads = [torch.from_numpy(g).clone() for g in golden_grads(z, meta, 1)]
    bad = [g.clone() for g in grads]
    bad[-1][17] = float('inf')
    s0 = dev.opt.grad_scaler.get_scale()
    dev.step([g * s0 for g in bad], max_norm=1e9)
    after = dev.tensors()
    for key in before:
        assert torch.equal(before[key], after[key]), key
    for k, b in dev.opt.bufs.items():
        assert torch.equal(b, arenas[k]), k
    assert dev.opt.step_count() == 0 and dev.opt.grad_scaler.found_inf()
    s1 = dev.opt.grad_scaler.get_scale()
    assert s1 == s0 / 2
    # the next finite step is a first step (power-of-two scale: unscaling is exact)
    dev.step([g * s1 for g in grads])
    twin.step(grads)
    assert dev.opt.step_count() == 1
    a, b = dev.tensors(), twin.tensors()
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ---- 5. one captured graph serves every step ----
@pytest.mark.parametrize('case,ctor', [('ranger', dict(lr=1e-2, weight_decay=1e-2, k=2)), ('diffmod', None)])
def test_capture_replays_equal_eager(hip_device, case, ctor):
    """Two eager steps, one capture, five replays == seven eager steps, bitwise: the rectification switch (step 6),
    every Lookahead step and the carried previous_grad happen inside replays of the same graph."""
    from ssseg.graph import StepGraph
    z, meta, _ = case_data(case)
    n = len(meta['sizes'])
    init = [torch.from_numpy(z[f'init_{i}']) for i in range(n)]
    ctor = ctor or meta['ctor']

    def run(graphed):
        dev = Device(meta['algo'], init, ctor, hip_device)
        flat = [dev.flat_grads(golden_grads(z, meta, t)) for t in range(1, 8)]

        def fn(g):
            dev.arena.grad.copy_(g)
            dev.opt.step(max_norm=3.0)
            return (dev.arena.data,)
        for t in range(2):
            fn(flat[t])
        if graphed:
            sg = StepGraph(fn, flat[2])
            for t in range(2, 7):
                sg(flat[t])
        else:
            for t in range(2, 7):
                fn(flat[t])
        torch.cuda.synchronize()
        return dev.tensors(), dev.opt.step_count()

    eager, n_e = run(False)
    graph, n_g = run(True)
    assert n_e == n_g == 7
    for key in eager:
        assert torch.equal(eager[key], graph[key]), key
        assert torch.isfinite(eager[key]).all()


# ---- 6. checkpoint interchange with the reference's format ----
@pytest.mark.parametrize('case', ('ranger', 'diffmod'))
def test_checkpoint_interchange(hip_device, case):
    z, meta, ref64 = case_data(case)
    n = len(meta['sizes'])
    dev = Device(meta['algo'], [torch.from_numpy(z[f'p_6_{i}']) for i in range(n)], meta['ctor'], hip_device)
    groups = dev.opt.state_dict()['param_groups']
    assert dev.opt.state_dict()['state'] == {}                       # not stepped yet: like the reference
    state = {i: dict({k: torch.from_numpy(z[f'{k}_6_{i}']).clone() for k in meta['state_keys']}, step=6)
             for i in range(n)}
    dev.opt.load_state_dict({'state': state, 'param_groups': groups})
    assert dev.opt.step_count() == 6
    worst, where, _ = run_golden(case, hip_device, first=7, dev=dev)
    assert worst <= 1.0, (worst, where)
    sd = dev.opt.state_dict()
    assert sorted(sd['state']) == list(range(n))
    for i in range(n):
        st = sd['state'][i]
        assert type(st['step']) is int and st['step'] == 12
        assert set(st) == set(meta['state_keys']) | {'step'}
        assert st['exp_avg'].shape == (meta['sizes'][i],)
    # per-parameter steps that disagree cannot come from dense gradients
    state[0]['step'] = 5
    with pytest.raises(ValueError, match='disagree'):
        dev.opt.load_state_dict({'state': state, 'param_groups': groups})


# ---- 7. through the trainer ----
def test_trainer_graph_vs_eager_with_ranger(hip_device):
    import bench
    import cowmix
    import losses
    import train
    from models import simple_unet
    from models.adapters import ListOutput
    from optimizers import Ranger
    from ssseg import arena
    from ssseg import nn as snn

    tcfg = dict(loss=losses.CalculateLoss([{'loss_fn': losses.DenseBinaryCrossEntropyLossWithLogits('mean'),
                                            'weight': [0.5]}]),
                virtual_batch_size_multiplier=1, use_semi_supervised=True, mask_proportion_range=(0.45, 0.55),
                sigma_range=(2, 4), confidence_threshold=0.5, consistency_loss_weight=10, ema_model_alpha=0.99,
                print_freq=10 ** 9, gradient_clip_value=5.0)
    steps = 6
    data = bench.synthetic_batches(steps, 2, 32, hip_device, 0)

    keep = []       # both runs' models stay alive: the trainer keys its per-model step counts on id()

    def run(graph):
        torch.manual_seed(0)
        student = ListOutput(simple_unet.UNet(2, 2, 8, 16)).to(hip_device)
        teacher = ListOutput(simple_unet.UNet(2, 2, 8, 16)).to(hip_device)
        teacher.load_state_dict(student.state_dict())
        for p in teacher.parameters():
            p.detach_()
        teacher.eval()
        arena.attach(student)
        arena.attach(teacher, with_grads=False)
        keep.extend([student, teacher])
        opt = Ranger(student.parameters(), lr=1e-3, k=2, weight_decay=5e-4)
        start = student._ssseg_arena.data.clone()
        for c in cowmix._DEVICE_RNG['ctr'].values():
            c.zero_()
        cfg = {'train': tcfg}
        was, cap0 = train._GRAPH['on'], train._GRAPH['captures']
        train._GRAPH['on'] = graph
        try:
            student.train()
            opt.zero_grad()
            out = [train.run_step(student, teacher, opt, *data[k], 30, k, cfg) for k in range(steps)]
            torch.cuda.synchronize()
        finally:
            train._GRAPH['on'] = was
            train.release_graphs()
        losses_ = [tuple(float(t) for t in o) for o in out]
        return losses_, student._ssseg_arena.data.clone(), start, train._GRAPH['captures'] - cap0, opt.step_count()

    prev = snn.compute_dtype()
    snn.set_compute_dtype(torch.bfloat16)
    try:
        l_e, p_e, _, caps_e, n_e = run(False)
        l_g, p_g, start, caps, n_g = run(True)
    finally:
        snn.set_compute_dtype(prev)
    assert caps >= 1 and caps_e == 0
    assert l_g == l_e, (l_g, l_e)
    assert n_g == n_e == steps - 1           # no optimizer step at step 0
    assert torch.equal(p_g, p_e)
    assert torch.isfinite(p_g).all() and not torch.equal(p_g, start)
