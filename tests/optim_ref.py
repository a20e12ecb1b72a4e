"""Per-tensor torch restatement of the fused optimizer family (Adam, AdaMod, DiffGrad, DiffMod, Ranger).

The yardstick of tests/test_optimizers_*.py: written from the papers (Adam arXiv:1412.6980, AdaMod
arXiv:1910.12249, diffGrad arXiv:1909.11015, RAdam arXiv:1908.03265, Lookahead arXiv:1907.08610) and from the
observable behaviour of the reference's classes.  Run in fp32 it issues the same torch ops in the same order as those
classes (tests/test_optimizers_host.py pins it to their recorded outputs with torch.equal; sqrt and exp are the
correctly rounded sqrt_rn / exp_rn below, on both sides); run in fp64 it is the "truth" that the device kernels and the
fp32 reference are both measured against.

    opt = RefOptim('ranger', [p0, p1, ...], dtype=torch.float64, lr=1e-2, weight_decay=1e-2, k=3)
    opt.step([g0, g1, ...])        # params / state are plain tensors in opt.params / opt.state[i]
"""
import math

import torch

DEFAULTS = {
    'adam': dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0),
    'adamod': dict(lr=1e-3, betas=(0.9, 0.999), beta3=0.999, eps=1e-8, weight_decay=0),
    'diffgrad': dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, version=0, weight_decay=0),
    'diffmod': dict(lr=1e-3, betas=(0.9, 0.999), beta3=0.999, version=0, eps=1e-8, weight_decay=0),
    'ranger': dict(lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0),
}
STATE_KEYS = {
    'adam': ('exp_avg', 'exp_avg_sq'),
    'adamod': ('exp_avg', 'exp_avg_sq', 'exp_avg_lr'),
    'diffgrad': ('exp_avg', 'exp_avg_sq', 'previous_grad'),
    'diffmod': ('exp_avg', 'exp_avg_sq', 'exp_avg_lr', 'previous_grad'),
    'ranger': ('exp_avg', 'exp_avg_sq', 'slow_buffer'),
}


_sqrt, _exp = torch.sqrt, torch.exp


def sqrt_rn(x):
    """Correctly rounded sqrt.  torch's CPU sqrt / exp of fp32 go through a vendor vector-math library whose last bit
    depends on the host CPU; evaluated in fp64 and rounded once they are the same on every machine.  The golden runs
    of the reference classes were recorded with these two in place of Tensor.sqrt / torch.exp (gen_golden_optim.py)."""
    return _sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else _sqrt(x)


def exp_rn(x):
    return _exp(x.double()).to(x.dtype) if x.dtype == torch.float32 else _exp(x)


def dfc(prev, g, version):
    """diffGrad friction coefficient from the change of the gradient."""
    d = prev - g
    if version == 0:
        d = abs(d)
    elif version == 2:
        d = .5 * abs(d)
    c = 1. / (1. + exp_rn(-d))
    return 9. * c - 4 if version == 2 else c


def replay(z, meta, dtype):
    """The recorded run of a golden case (tests/golden/optim_<case>.npz) through the restatement:
    ({(key, step, tensor index): tensor} at the stored steps with key 'p' or a state key, the RefOptim)."""
    n = len(meta['sizes'])
    opt = RefOptim(meta['algo'], [torch.from_numpy(z[f'init_{i}']) for i in range(n)], dtype=dtype, **meta['hyper'])
    out = {}
    for t in range(1, meta['T'] + 1):
        opt.step([torch.from_numpy(z[f'grad_{t}_{i}']) for i in range(n)])
        if t in meta['steps']:
            for i in range(n):
                out['p', t, i] = opt.params[i].clone()
                for k in meta['state_keys']:
                    out[k, t, i] = opt.state[i][k].clone()
    return out, opt


class RefOptim:
    def __init__(self, algo, params, dtype=torch.float32, **hyper):
        self.algo, self.dtype = algo, dtype
        self.h = dict(DEFAULTS[algo], **hyper)
        self.params = [p.detach().clone().to(dtype) for p in params]
        self.state = [{k: torch.zeros_like(p) for k in STATE_KEYS[algo]} for p in self.params]
        self.t = 0
        self.trace = []            # ranger: (rectified, lookahead) per step

    def step(self, grads):
        self.t += 1
        for p, st, g in zip(self.params, self.state, grads):
            getattr(self, '_' + self.algo)(p, st, g.detach().clone().to(self.dtype))

    # ---- shared pieces ----
    def _moments(self, st, g, v_first=False):
        b1, b2 = self.h['betas']
        m, v = st['exp_avg'], st['exp_avg_sq']
        if v_first:
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            m.mul_(b1).add_(g, alpha=1 - b1)
        else:
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
        return m, v

    def _bias(self):
        b1, b2 = self.h['betas']
        return 1 - b1 ** self.t, 1 - b2 ** self.t

    def _momental_bound(self, st, step_size, denom):
        b3 = self.h['beta3']
        eta = torch.full_like(denom, step_size).div_(denom)
        st['exp_avg_lr'].mul_(b3).add_(eta, alpha=1 - b3)
        return torch.min(eta, st['exp_avg_lr'])

    # ---- the five algorithms ----
    def _adam(self, p, st, g):
        h = self.h
        if h['weight_decay'] != 0:
            g = g.add(p, alpha=h['weight_decay'])
        b1, b2 = h['betas']
        m, v = st['exp_avg'], st['exp_avg_sq']
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = self._bias()
        denom = (sqrt_rn(v) / (bc2 ** 0.5)).add_(h['eps'])
        p.addcdiv_(m, denom, value=-(h['lr'] / bc1))

    def _adamod(self, p, st, g):
        h = self.h
        m, v = self._moments(st, g)
        denom = sqrt_rn(v).add_(h['eps'])
        bc1, bc2 = self._bias()
        step_size = h['lr'] * math.sqrt(bc2) / bc1
        if h['weight_decay'] != 0:
            p.add_(p, alpha=-h['weight_decay'] * h['lr'])
        bounded = self._momental_bound(st, step_size, denom)
        p.add_(-bounded.mul_(m))

    def _diffgrad(self, p, st, g):
        h = self.h
        if h['weight_decay'] != 0:
            g.add_(p, alpha=h['weight_decay'])
        m, v = self._moments(st, g)
        denom = sqrt_rn(v).add_(h['eps'])
        bc1, bc2 = self._bias()
        c = dfc(st['previous_grad'], g, h['version'])
        st['previous_grad'] = g
        step_size = h['lr'] * math.sqrt(bc2) / bc1
        p.addcdiv_(m * c, denom, value=-step_size)

    def _diffmod(self, p, st, g):
        h = self.h
        m, v = self._moments(st, g)
        denom = sqrt_rn(v).add_(h['eps'])
        bc1, bc2 = self._bias()
        step_size = h['lr'] * math.sqrt(bc2) / bc1
        c = dfc(st['previous_grad'], g, h['version'])
        st['previous_grad'] = g
        if h['weight_decay'] != 0:
            p.add_(p, alpha=-h['weight_decay'] * h['lr'])
        bounded = self._momental_bound(st, step_size, denom)
        p.add_(-bounded.mul_(m * c))

    def _ranger(self, p, st, g):
        h = self.h
        b1, b2 = h['betas']
        t = self.t
        if t == 1:
            st['slow_buffer'].copy_(p)          # the parameters as they stand on entry to the first step
        m, v = self._moments(st, g, v_first=True)
        beta2_t = b2 ** t
        n_max = 2 / (1 - b2) - 1
        n_sma = n_max - 2 * t * beta2_t / (1 - beta2_t)
        rect = n_sma > h['N_sma_threshhold']
        if rect:
            step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max /
                                  (n_max - 2)) / (1 - b1 ** t)
        else:
            step_size = 1.0 / (1 - b1 ** t)
        if h['weight_decay'] != 0:
            p.add_(p, alpha=-h['weight_decay'] * h['lr'])
        if rect:
            p.addcdiv_(m, sqrt_rn(v).add_(h['eps']), value=-step_size * h['lr'])
        else:
            p.add_(m, alpha=-step_size * h['lr'])
        look = t % h['k'] == 0
        if look:
            slow = st['slow_buffer']
            slow.add_(p - slow, alpha=h['alpha'])
            p.copy_(slow)
        if p is self.params[0]:
            self.trace.append((rect, look))
