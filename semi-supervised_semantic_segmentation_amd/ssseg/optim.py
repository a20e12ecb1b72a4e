"""SGD with momentum / weight decay and fused gradient clipping over a flat arena.

Replaces torch.optim.SGD (reference default_config.py:151-154) + clip_grad_norm_ (train.py:122):
one squared-norm reduction + one fused clip/weight-decay/momentum/update launch for the whole model
instead of ~4 launches per parameter tensor.  Subclasses torch.optim.Optimizer so LR schedulers and
state_dict()/load_state_dict() work (momentum buffers are exposed per parameter as views).
"""
import torch

from . import arena as _arena
from . import native as N
from . import ops


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if dampening != 0 or nesterov:
            raise NotImplementedError('ssseg SGD: dampening / nesterov')
        params = list(params)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                      nesterov=False))
        ps = [p for g in self.param_groups for p in g['params']]
        arenas = {id(getattr(p, '_ssseg_arena', None)) for p in ps}
        a = getattr(ps[0], '_ssseg_arena', None)
        if a is None or len(arenas) != 1 or len(self.param_groups) != 1 or len(ps) != len(a.params):
            raise RuntimeError('ssseg SGD needs one param group covering a whole flat arena (ssseg.arena.attach)')
        self.arena = a
        self.buf = torch.zeros_like(a.data) if momentum else None
        self._first = True
        self._sq = torch.zeros(1, dtype=torch.float32, device=a.data.device)
        self.grad_scaler = None     # ssseg.amp.GradScaler in the fp16 compute mode (loss-scaled gradients)
        if self.buf is not None:
            for p, o in zip(a.params, a.offsets):
                self.state[p]['momentum_buffer'] = self.buf[o:o + p.numel()].view_as(p)

    def zero_grad(self, set_to_none=False):
        self.arena.zero_grad()

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict, then the loaded momentum buffers are copied into the flat
        momentum arena and the per-parameter state entries point back at its views (resume,
        distributed_trainer.py:64): the next step continues the momentum like torch.optim.SGD does."""
        super().load_state_dict(state_dict)
        loaded = False
        with torch.no_grad():
            for p, o in zip(self.arena.params, self.arena.offsets):
                st = self.state.get(p, {})
                mb = st.get('momentum_buffer') if isinstance(st, dict) else None
                if self.buf is None:
                    continue
                view = self.buf[o:o + p.numel()].view_as(p)
                if mb is not None:
                    view.copy_(mb.to(view.device, view.dtype))
                    loaded = True
                self.state[p]['momentum_buffer'] = view
        if loaded:
            self._first = False

    @torch.no_grad()
    def step(self, closure=None, max_norm=0.0, fused=None):
        """max_norm > 0 clips the global gradient L2 norm first (clip_grad_norm_, train.py:122).
        fused = (plan, teacher arena, alpha) with plan = param_step.plan_for(student, teacher, self): this step, the
        teacher's EMA, the repack of both models and the gradient clear as ONE launch (ssseg.param_step)."""
        if fused is not None:
            from . import param_step as _ps
            plan, teacher_arena, alpha = fused
            _ps.step(plan, self, teacher_arena, max_norm, alpha)
            return None
        g = self.param_groups[0]
        sc = self.grad_scaler
        if (max_norm and max_norm > 0) or sc is not None:
            N.call('ssseg_zero', N.dev_ptr(self._sq), 4, N.stream())
            ops.sqnorm_(self.arena.grad, self._sq)
        ops.sgd_step_(self.arena.data, self.arena.grad, self.buf, None, g['lr'], g['momentum'], g['weight_decay'],
                      max_norm or 0.0, self._sq if (max_norm or sc is not None) else None, self._first,
                      sc.state if sc is not None else None)
        if sc is not None:
            sc.update(self._sq)
        self._first = False
        return None


def _whole_arena(params):
    """The flat arena that `params` cover completely, else None."""
    a = getattr(params[0], '_ssseg_arena', None) if params else None
    if a is None or len(params) != len(a.params) or any(getattr(p, '_ssseg_arena', None) is not a for p in params):
        return None
    return a


class FusedOptimizer(torch.optim.Optimizer):
    """Base of the fused Adam family (Adam here; Ranger, AdaMod, DiffGrad, DiffMod in the top-level `optimizers`
    package): clip + update of the whole model in two launches with fixed arguments (ssseg_optim_prepare,
    ssseg_optim_step).

    Same contract as SGD above: one param group covering a whole flat arena.  The state arenas the algorithm needs
    (STATE_KEYS, the reference's names) are flat tensors viewed per parameter in self.state; the step counter lives on
    the device (state block [0]) and all state starts at zero, so the first step is no special case and every step,
    Ranger's rectification switch and Lookahead included, replays from one captured graph.  state_dict() /
    load_state_dict() speak the reference classes' format ('step' a Python int per parameter)."""
    MODE = None
    STATE_KEYS = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, defaults):
        params = list(params)
        super().__init__(params, defaults)
        ps = [p for g in self.param_groups for p in g['params']]
        a = _whole_arena(ps)
        if a is None or len(self.param_groups) != 1:
            raise RuntimeError(f'ssseg {type(self).__name__} needs one param group covering a whole flat arena '
                               '(ssseg.arena.attach)')
        self.arena = a
        self.bufs = {k: torch.zeros_like(a.data) for k in self.STATE_KEYS}
        self._state = torch.zeros(N.OPT_STATE_DOUBLES, dtype=torch.float64, device=a.data.device)
        self._sq = torch.zeros(1, dtype=torch.float32, device=a.data.device)
        self.version = 0
        self.grad_scaler = None     # ssseg.amp.GradScaler in the fp16 compute mode (loss-scaled gradients)
        self._point_views()

    def _point_views(self):
        for p, o in zip(self.arena.params, self.arena.offsets):
            for k, buf in self.bufs.items():
                self.state[p][k] = buf[o:o + p.numel()].view_as(p)

    def zero_grad(self, set_to_none=False):
        self.arena.zero_grad()

    def step_count(self):
        """The device step counter (a host sync: checkpoint time only)."""
        return int(self._state[0].item())

    def state_dict(self):
        t = self.step_count()
        for p in self.arena.params:
            self.state[p]['step'] = t
        sd = super().state_dict()
        if t == 0:
            sd['state'] = {}        # like a reference optimizer that has not stepped (its state is created lazily)
        return sd

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict, then the loaded tensors are copied into the flat state arenas, the
        per-parameter entries point back at their views and the device counter is set.  Raises if the per-parameter
        steps disagree (dense gradients step every parameter together)."""
        super().load_state_dict(state_dict)
        steps = set()
        with torch.no_grad():
            # assembled aside, then copied over the arenas in place (captured graphs hold their addresses; the loaded
            # tensors may be this optimizer's own views)
            fresh = {k: torch.zeros_like(buf) for k, buf in self.bufs.items()}
            for p, o in zip(self.arena.params, self.arena.offsets):
                st = self.state.get(p, {})
                steps.add(int(st.get('step', 0)))
                for k, buf in fresh.items():
                    t = st.get(k)
                    if t is not None:
                        buf[o:o + p.numel()].view_as(p).copy_(t.to(buf.device, buf.dtype))
            if len(steps) > 1:
                raise ValueError(f'ssseg {type(self).__name__}: the loaded per-parameter steps disagree: '
                                 f'{sorted(steps)}')
            for k, buf in self.bufs.items():
                buf.copy_(fresh[k])
            self._state.zero_()
            self._state[0] = float(steps.pop() if steps else 0)
        self._point_views()

    def _hyper(self, g):
        """(beta3, k, N_sma threshold, alpha) of the param group; the algorithms without them use the neutral values."""
        return g.get('beta3', 0.0), g.get('k', 1), g.get('N_sma_threshhold', 0.0), g.get('alpha', 0.0)

    @torch.no_grad()
    def step(self, closure=None, max_norm=0.0):
        """max_norm > 0 clips the global gradient L2 norm first (clip_grad_norm_, train.py:122)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        sc = self.grad_scaler
        max_norm = max_norm or 0.0
        need_norm = max_norm > 0 or sc is not None
        if need_norm:
            N.call('ssseg_zero', N.dev_ptr(self._sq), 4, N.stream())
            ops.sqnorm_(self.arena.grad, self._sq)
        b1, b2 = g['betas']
        b3, k, thr, alpha = self._hyper(g)
        ops.optim_prepare_(self._state, self.MODE, g['lr'], b1, b2, g['weight_decay'], max_norm, k, thr,
                           self._sq if need_norm else None, sc.state if sc is not None else None)
        ops.optim_step_(self.arena.data, self.arena.grad, self.bufs['exp_avg'], self.bufs['exp_avg_sq'],
                        self.bufs.get('exp_avg_lr'), self.bufs.get('previous_grad'), self.bufs.get('slow_buffer'),
                        self.MODE, self.version, b1, b2, b3, g['eps'], g['weight_decay'], alpha, self._state)
        if sc is not None:
            sc.update(self._sq)
        return loss


def _check_adam_family(lr, eps, betas):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))


class Adam(FusedOptimizer):
    """torch.optim.Adam (L2 weight decay added to the gradient; no amsgrad, not maximize)."""
    MODE = N.OPT_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError('ssseg Adam: amsgrad / maximize')
        _check_adam_family(lr, eps, betas)
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False))


_ADAM_KEYWORDS = {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize'}


def _fusable_adam(kw, params):
    if set(kw) - _ADAM_KEYWORDS or kw.get('amsgrad') or kw.get('maximize'):
        return False
    if any(isinstance(kw.get(k), torch.Tensor) for k in ('lr', 'eps', 'weight_decay')) or \
            any(isinstance(b, torch.Tensor) for b in kw.get('betas', ())):
        return False
    return bool(params) and not isinstance(params[0], dict) and _whole_arena(params) is not None


def from_config(factory, params):
    """Map a reference config's optimizer factory (functools.partial(torch.optim.SGD, ...)) to ssseg SGD, and
    torch.optim.Adam to the fused Adam where its keywords and parameters allow (a whole flat arena; no amsgrad)."""
    fn = getattr(factory, 'func', factory)
    if fn is torch.optim.SGD or fn is SGD:
        kw = dict(getattr(factory, 'keywords', {}) or {})
        return SGD(params, **kw)
    if fn is torch.optim.Adam and not getattr(factory, 'args', ()):
        kw = dict(getattr(factory, 'keywords', {}) or {})
        params = list(params)
        if _fusable_adam(kw, params):
            return Adam(params, **kw)
    return factory(params=params)
