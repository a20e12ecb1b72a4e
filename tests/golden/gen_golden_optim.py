"""Golden vectors of the reference's optimizers (optimizers/{ranger,adamod,diffgrad,diffmod}.py) and torch.optim.Adam.

RUNS ONLY IN THE BUILD CONTAINER, on CPU, where the reference is mounted read-only (see gen_golden.py).  It imports
the reference's own classes, drives them for T steps with recorded random gradients over tensors of 1, 3, 7, 64 and
1030 elements and writes tests/golden/optim_<case>.npz: the initial parameters, every step's gradients, and the
parameters plus every state tensor after the stored steps.  The constructor signatures (names, defaults) are recorded
as data too.  Nothing of the reference travels with the files.

While the classes step, Tensor.sqrt and torch.exp are the correctly rounded sqrt_rn / exp_rn of tests/optim_ref.py:
torch's own CPU versions go through a vendor vector-math library whose last bit depends on the host CPU, so a run
recorded with them could be reproduced bit for bit (tests/test_optimizers_host.py) only on the machine that made it.

  keys:  init_<i>  grad_<t>_<i>  p_<s>_<i>  <state key>_<s>_<i>  (t = 1..T, s in `steps`, i = tensor index)
         meta (JSON: case, algo, hyper-parameters, constructor keywords, T, steps, sizes, state keys, signature)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_optim.py
"""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(OUT))

import torch  # noqa: E402

from optim_ref import exp_rn, sqrt_rn  # noqa: E402  (tests/optim_ref.py)

from optimizers.adamod import AdaMod  # noqa: E402  (reference)
from optimizers.diffgrad import DiffGrad  # noqa: E402
from optimizers.diffmod import DiffMod  # noqa: E402
from optimizers.ranger import Ranger  # noqa: E402

T = 12
STEPS = (1, 5, 6, 7, 12)
SIZES = (1, 3, 7, 64, 1030)
COMMON = dict(lr=1e-2, weight_decay=1e-2)

CASES = {
    'ranger': ('ranger', Ranger, dict(k=3)),
    'adamod': ('adamod', AdaMod, {}),
    'diffgrad_v0': ('diffgrad', DiffGrad, dict(version=0)),
    'diffgrad_v2': ('diffgrad', DiffGrad, dict(version=2)),
    'diffmod': ('diffmod', DiffMod, dict(version=0, len_memory=10)),
    'adam': ('adam', torch.optim.Adam, {}),
}
STATE_KEYS = {
    'adam': ('exp_avg', 'exp_avg_sq'),
    'adamod': ('exp_avg', 'exp_avg_sq', 'exp_avg_lr'),
    'diffgrad': ('exp_avg', 'exp_avg_sq', 'previous_grad'),
    'diffmod': ('exp_avg', 'exp_avg_sq', 'exp_avg_lr', 'previous_grad'),
    'ranger': ('exp_avg', 'exp_avg_sq', 'slow_buffer'),
}


def signature(cls):
    """[(name, default or None)] of the constructor after (self, params)."""
    ps = list(inspect.signature(cls.__init__).parameters.values())[2:]
    return [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in ps]


@contextlib.contextmanager
def exact_elementary():
    """Tensor.sqrt / torch.exp -> their correctly rounded forms while the reference classes step."""
    sqrt0, exp0 = torch.Tensor.sqrt, torch.exp
    torch.Tensor.sqrt, torch.exp = sqrt_rn, exp_rn
    try:
        yield
    finally:
        torch.Tensor.sqrt, torch.exp = sqrt0, exp0


def run_case(case, seed):
    algo, cls, extra = CASES[case]
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in SIZES]
    out = {f'init_{i}': p.detach().numpy().copy() for i, p in enumerate(params)}
    with contextlib.redirect_stdout(io.StringIO()):          # DiffMod prints its memory length
        opt = cls(params, **COMMON, **extra)
    rectified, lookahead = [], 0
    for t in range(1, T + 1):
        for i, p in enumerate(params):
            gr = torch.randn(p.shape, generator=g) * (0.5 + 0.5 * torch.rand(1, generator=g))
            out[f'grad_{t}_{i}'] = gr.numpy().copy()
            p.grad = gr.clone()        # a fresh tensor per step: an aliased previous_grad keeps the old values
        with exact_elementary():
            opt.step()
        if algo == 'ranger':
            n_sma = opt.radam_buffer[t % 10][1]
            rectified.append(bool(n_sma > opt.N_sma_threshhold))
            if t % opt.k == 0:
                assert all(torch.equal(p.data, opt.state[p]['slow_buffer']) for p in params)
                lookahead += 1
        if t in STEPS:
            for i, p in enumerate(params):
                out[f'p_{t}_{i}'] = p.detach().numpy().copy()
                st = opt.state[p]
                assert int(st['step']) == t
                for k in STATE_KEYS[algo]:
                    out[f'{k}_{t}_{i}'] = st[k].detach().numpy().copy()
    if algo == 'ranger':
        # both RAdam branches and at least three Lookahead interpolations inside the recorded run
        assert any(rectified) and not all(rectified), rectified
        assert lookahead >= 3, lookahead
    hyper = dict(COMMON, **extra)
    if 'len_memory' in hyper:
        hyper['beta3'] = 1 - (1 / hyper.pop('len_memory'))
    meta = dict(case=case, algo=algo, hyper=hyper, ctor=dict(COMMON, **extra), T=T, steps=list(STEPS),
                sizes=list(SIZES),
                state_keys=list(STATE_KEYS[algo]), rectified=rectified,
                signature=None if cls is torch.optim.Adam else signature(cls), cls=cls.__name__)
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f'optim_{case}.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes, rectified={rectified}')


if __name__ == '__main__':
    for n, case in enumerate(CASES):
        run_case(case, 100 + n)
