"""Host-side checks of the fused optimizer family (no GPU): the `optimizers` package keeps the reference's import
paths, signatures and ValueError checks; the torch restatement used as the GPU tests' yardstick (tests/optim_ref.py)
reproduces the reference classes' recorded outputs bit for bit on any host (the runs were recorded with correctly
rounded sqrt / exp, see optim_ref.sqrt_rn); from_config maps torch.optim.Adam; the checkpoint format round-trips."""
import importlib
import inspect
import json
from functools import partial

import pytest
import torch

from conftest import golden
from optim_ref import replay

CASES = ('ranger', 'adamod', 'diffgrad_v0', 'diffgrad_v2', 'diffmod', 'adam')
MODULES = {'Ranger': 'optimizers.ranger', 'AdaMod': 'optimizers.adamod', 'DiffGrad': 'optimizers.diffgrad',
           'DiffMod': 'optimizers.diffmod'}


def load_case(case):
    z = golden(f'optim_{case}.npz')
    return z, json.loads(str(z['meta']))


def _listify(x):
    return [_listify(v) for v in x] if isinstance(x, (list, tuple)) else x


@pytest.mark.parametrize('case', ('ranger', 'adamod', 'diffgrad_v0', 'diffmod'))
def test_package_imports_with_the_reference_signatures(case):
    _, meta = load_case(case)
    mod = importlib.import_module(MODULES[meta['cls']])
    cls = getattr(mod, meta['cls'])
    import optimizers
    assert getattr(optimizers, meta['cls']) is cls and issubclass(cls, torch.optim.Optimizer)
    ps = list(inspect.signature(cls.__init__).parameters.values())[2:]
    got = [[p.name, None if p.default is inspect.Parameter.empty else _listify(p.default)] for p in ps]
    assert got == meta['signature']


def _arena_model(device='cpu'):
    from ssseg import arena
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2)).to(device)
    arena.attach(m)
    return m


@pytest.mark.parametrize('name,kw', [
    ('Ranger', dict(alpha=1.5)), ('Ranger', dict(alpha=-0.1)), ('Ranger', dict(k=0)), ('Ranger', dict(lr=0)),
    ('Ranger', dict(eps=0)),
    ('AdaMod', dict(lr=-1e-3)), ('AdaMod', dict(eps=-1e-8)), ('AdaMod', dict(betas=(1.0, 0.999))),
    ('AdaMod', dict(betas=(0.9, 1.0))), ('AdaMod', dict(beta3=1.0)),
    ('DiffGrad', dict(lr=-1e-3)), ('DiffGrad', dict(eps=-1e-8)), ('DiffGrad', dict(betas=(-0.1, 0.999))),
    ('DiffGrad', dict(betas=(0.9, 1.5))),
    ('DiffMod', dict(lr=-1e-3)), ('DiffMod', dict(eps=-1e-8)), ('DiffMod', dict(betas=(1.0, 0.999))),
    ('DiffMod', dict(betas=(0.9, -1.0))), ('DiffMod', dict(len_memory=0.5)),
])
def test_reference_value_errors(name, kw):
    import optimizers
    with pytest.raises(ValueError):
        getattr(optimizers, name)(_arena_model().parameters(), **kw)


def test_needs_a_whole_arena():
    import optimizers
    m = torch.nn.Linear(3, 5)
    with pytest.raises(RuntimeError, match='whole flat arena'):
        optimizers.Ranger(m.parameters())
    m = _arena_model()
    with pytest.raises(RuntimeError, match='whole flat arena'):
        optimizers.DiffMod(list(m.parameters())[:2])
    opt = optimizers.DiffMod(m.parameters(), len_memory=10)
    assert opt.param_groups[0]['beta3'] == 1 - (1 / 10)
    assert not hasattr(opt, '_first')
    p = next(m.parameters())
    assert set(opt.state[p]) == {'exp_avg', 'exp_avg_sq', 'exp_avg_lr', 'previous_grad'}
    assert opt.state[p]['exp_avg'].shape == p.shape
    assert set(opt.bufs) == set(opt.STATE_KEYS)       # only the arenas its algorithm needs
    assert set(optimizers.Ranger(_arena_model().parameters()).bufs) == {'exp_avg', 'exp_avg_sq', 'slow_buffer'}


@pytest.mark.parametrize('case', CASES)
def test_fp32_restatement_equals_the_reference(case):
    z, meta = load_case(case)
    out, opt = replay(z, meta, torch.float32)
    assert len(out) == len(meta['steps']) * len(meta['sizes']) * (1 + len(meta['state_keys']))
    for (k, t, i), v in out.items():
        assert torch.equal(v, torch.from_numpy(z[f'{k}_{t}_{i}'])), (k, t, i)
    if meta['algo'] == 'ranger':
        rect = [r for r, _ in opt.trace]
        assert rect == meta['rectified'] and any(rect) and not all(rect)
        assert sum(l for _, l in opt.trace) >= 3


def test_from_config_maps_adam():
    from ssseg import optim
    m = _arena_model()
    opt = optim.from_config(partial(torch.optim.Adam, lr=1e-3, weight_decay=1e-4), m.parameters())
    assert type(opt) is optim.Adam and opt.param_groups[0]['weight_decay'] == 1e-4
    assert isinstance(opt, optim.FusedOptimizer) and set(opt.bufs) == {'exp_avg', 'exp_avg_sq'}
    # not arena-backed, or keywords the kernel does not implement: torch's own class, as before
    plain = torch.nn.Linear(3, 5)
    assert type(optim.from_config(partial(torch.optim.Adam, lr=1e-3), plain.parameters())) is torch.optim.Adam
    assert type(optim.from_config(partial(torch.optim.Adam, lr=1e-3, amsgrad=True),
                                  _arena_model().parameters())) is torch.optim.Adam
    assert type(optim.from_config(partial(torch.optim.AdamW, lr=1e-3),
                                  _arena_model().parameters())) is torch.optim.AdamW


def test_state_dict_round_trip_on_the_host():
    """The checkpoint format needs no kernel: 'step' an int per parameter, the reference's keys, views re-pointed at
    the arenas after a load -- also when an optimizer loads its own state_dict (the loaded tensors are its views)."""
    import optimizers
    a = optimizers.DiffMod(_arena_model().parameters(), len_memory=10)
    assert a.state_dict()['state'] == {}
    for buf in a.bufs.values():
        buf.copy_(torch.randn_like(buf))
    a._state[0] = 3.0
    sd = a.state_dict()
    assert all(type(s['step']) is int and s['step'] == 3 for s in sd['state'].values()) and len(sd['state']) == 4
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq', 'exp_avg_lr', 'previous_grad'}
    want = {k: b.clone() for k, b in a.bufs.items()}
    a.load_state_dict(a.state_dict())
    b = optimizers.DiffMod(_arena_model().parameters(), len_memory=10)
    b.load_state_dict(sd)
    for o in (a, b):
        assert o.step_count() == 3
        for (pa, oa), pb in zip(zip(a.arena.params, a.arena.offsets), o.arena.params):
            for k in want:
                assert torch.equal(o.state[pb][k], want[k][oa:oa + pa.numel()].view_as(pa)), k
                assert o.state[pb][k].data_ptr() >= o.bufs[k].data_ptr()
    sd['state'][1]['step'] = 4
    with pytest.raises(ValueError, match='disagree'):
        b.load_state_dict(sd)


def test_grad_scaler_attaches_to_the_fused_family_only():
    import distributed_trainer
    import optimizers
    from ssseg import amp
    opt = optimizers.Ranger(_arena_model().parameters())
    sc = distributed_trainer.attach_grad_scaler(opt, torch.device('cpu'))
    assert isinstance(sc, amp.GradScaler) and opt.grad_scaler is sc
    with pytest.raises(NotImplementedError):
        distributed_trainer.attach_grad_scaler(torch.optim.Adam(torch.nn.Linear(2, 2).parameters()), torch.device('cpu'))


def test_example_config_imports_like_the_reference_default():
    import os
    import config
    import train
    cfg = config.fromfile(os.path.join(os.path.dirname(train.__file__), 'configs', 'c1_simple_unet_ranger.py'))
    from optimizers.ranger import Ranger
    assert cfg['train']['optimizer'].func is Ranger
