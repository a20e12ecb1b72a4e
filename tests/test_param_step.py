"""ssseg_param_step (csrc/param_step.hip) against the launches it replaces, bit for bit.

A synthetic arena (param_step_cases.py: conv weights (8,8,1,1), (64,8,7,7), (72,40,3,3) and a ConvTranspose2d
(24,16,4,4) with its four phase packs, 1 / 2 / 4 / 10 packs per weight, ranges of 1, 255 and 1027 elements between
them) is stepped twice from the same state: once by ssseg_sqnorm_accum + ssseg_sgd_step + gradient clear +
ssseg_weight_pack_batch (student) + ssseg_ema_update + ssseg_weight_pack_batch (teacher), once by the fused launch.
p, buf, ema, g and every pack must have the same raw bits.  p and buf are also held to sgd_ref and ema to ema_ref
(tests/exact_step.py), the restatements the separate kernels are pinned to.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import exact_step as E
import param_step_cases as cases

pytestmark = pytest.mark.gpu

LR, MOM, ALPHA = 0.05, 0.9, 0.99
SGD, EMA, CLEAR = 1, 2, 4


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


class World:
    """arenas, packs and both descriptor tables on the device; state() / restore() snapshot everything a step writes"""

    def __init__(self, dev):
        self.dev = dev
        slots, self.numel = cases.layout()
        self.slots = slots
        g = torch.Generator().manual_seed(20)
        rnd = lambda: torch.randn(self.numel, generator=g)  # noqa: E731  (gaps and alignment pads are random too)
        grad = rnd() * 3
        grad[0] = 1.0                                      # g'[0] is the coefficient the device applied
        self.t = {'p': rnd().to(dev), 'g': grad.to(dev), 'buf': rnd().to(dev), 'ema': rnd().to(dev)}
        self.packs, rows = [], {0: [], 1: []}
        weights = []
        for name, off, n, shape, packs in slots:
            if shape is None:
                continue
            plist = []
            for teacher, spec in packs:
                t = torch.full((cases.pack_numel(spec),), -7.0, dtype=torch.bfloat16, device=dev)   # a value no pack holds
                self.packs.append(t)
                src = self.t['ema' if teacher else 'p']
                rows[teacher].append((src.data_ptr() + 4 * off, t.data_ptr()) + spec)
                plist.append((t.data_ptr(), teacher, spec))
            weights.append((off, shape, plist))
        self.weights = weights
        self.tables = {k: torch.tensor(v, dtype=torch.int64).to(dev) for k, v in rows.items()}
        self.nrows = {k: len(v) for k, v in rows.items()}
        self.sq = torch.zeros(1, device=dev)
        self.plan = self.table(weights)
        self.initial = self.state()

    def table(self, weights):
        from ssseg import param_step
        descs, packs = param_step.group(self.numel, weights)
        return (torch.tensor(descs, dtype=torch.int64).to(self.dev), len(descs),
                torch.tensor(packs, dtype=torch.int64).to(self.dev))

    def state(self):
        return {k: v.clone() for k, v in self.t.items()}, [p.clone() for p in self.packs]

    def restore(self, st=None):
        arenas, packs = st or self.initial
        for k, v in arenas.items():
            self.t[k].copy_(v)
        for p, q in zip(self.packs, packs):
            p.copy_(q)

    def norm(self):
        return float(self.initial[0]['g'].double().pow(2).sum().sqrt())

    # -- the separate sequence ---------------------------------------------------------------------------------------
    def separate(self, max_norm, first, wd, flags, amp=None, sq=None):
        from ssseg import native as N
        from ssseg import ops
        t = self.t
        clipped = None
        if flags & SGD:
            self._sqnorm(max_norm, amp, sq)
            ops.sgd_step_(t['p'], t['g'], t['buf'], None, LR, MOM, wd, max_norm,
                          self.sq if (max_norm > 0 or amp is not None) else None, first, amp)
            clipped = t['g'].clone()
            if flags & CLEAR:
                N.call('ssseg_zero', N.dev_ptr(t['g']), self.numel * 4, N.stream())
            N.call('ssseg_weight_pack_batch', N.dev_ptr(self.tables[0]), self.nrows[0], N.BF16, N.stream())
        if flags & EMA:
            ops.ema_update_(t['ema'], t['p'], ALPHA)
            N.call('ssseg_weight_pack_batch', N.dev_ptr(self.tables[1]), self.nrows[1], N.BF16, N.stream())
        return clipped

    def _sqnorm(self, max_norm, amp, sq):
        from ssseg import native as N
        from ssseg import ops
        if sq is not None:
            self.sq.fill_(sq)
        elif max_norm > 0 or amp is not None:
            N.call('ssseg_zero', N.dev_ptr(self.sq), 4, N.stream())
            ops.sqnorm_(self.t['g'], self.sq)

    # -- the fused launch --------------------------------------------------------------------------------------------
    def fused(self, max_norm, first, wd, flags, amp=None, sq=None, plan=None):
        from ssseg import param_step
        t = self.t
        if flags & SGD:
            self._sqnorm(max_norm, amp, sq)
        param_step.launch(plan or self.plan, t['p'], t['g'], t['buf'], t['ema'], LR, MOM, wd, max_norm,
                          self.sq if (max_norm > 0 or amp is not None) else None, first, ALPHA, flags, amp)


@pytest.fixture(scope='module')
def world(hip_device):
    return World(hip_device)


def _same(a, b, what):
    (ta, pa), (tb, pb) = a, b
    for k in ta:
        E.same_bits(_bits(ta[k]), _bits(tb[k]), f'{what}: {k}')
    for i, (x, y) in enumerate(zip(pa, pb)):
        E.same_bits(_bits(x), _bits(y), f'{what}: pack {i}')


def _differs(a, b):
    return any(not np.array_equal(_bits(a[0][k]), _bits(b[0][k])) for k in a[0])


def _run_both(world, max_norm, first, wd, flags, amp=None, sq=None):
    world.restore()
    clipped = world.separate(max_norm, first, wd, flags, amp, sq)
    want = world.state()
    world.restore()
    world.fused(max_norm, first, wd, flags, amp, sq)
    got = world.state()
    torch.cuda.synchronize()
    return want, got, clipped


@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('first', [True, False], ids=['first', 'later'])
@pytest.mark.parametrize('clip', ['off', 'above', 'below'])
def test_fused_equals_the_separate_sequence(world, clip, first, wd):
    max_norm = float(np.float32({'off': 0.0, 'above': 2.0, 'below': 0.25}[clip] * world.norm()))
    want, got, clipped = _run_both(world, max_norm, first, wd, SGD | EMA | CLEAR)
    _same(want, got, f'{clip}/{first}/{wd}')
    # the step did something everywhere: every arena moved, g is clear, no pack still holds its fill value
    init = world.initial[0]
    for k in ('p', 'buf', 'ema'):
        assert float((got[0][k] != init[k]).float().mean()) > 0.99, k
    assert not bool(got[0]['g'].any())
    for i, p in enumerate(got[1]):
        assert not bool((p == -7.0).any()), f'pack {i} not fully written'
    # and it is the arithmetic the separate kernels are pinned to (exact_step.sgd_ref / ema_ref), with the
    # coefficient the separate launch applied (g[0] = 1)
    coef = float(clipped[0])
    assert (coef == 1.0) == (clip != 'below')
    h = {k: v.cpu().numpy() for k, v in init.items()}
    rp, _, rb, _ = E.sgd_ref(h['p'], h['g'], h['buf'], coef, LR, MOM, wd, first, False)
    E.same_bits(got[0]['p'].cpu().numpy(), rp, 'p vs sgd_ref')
    E.same_bits(got[0]['buf'].cpu().numpy(), rb, 'buf vs sgd_ref')
    E.same_bits(got[0]['ema'].cpu().numpy(), E.ema_ref(h['ema'], rp, ALPHA), 'ema vs ema_ref')


def test_without_clear_the_gradient_is_left_clipped(world):
    want, got, clipped = _run_both(world, float(np.float32(0.25 * world.norm())), False, 5e-4, SGD | EMA)
    _same(want, got, 'no clear')
    E.same_bits(_bits(got[0]['g']), _bits(clipped), 'g left clipped')
    assert bool(got[0]['g'].any())


def test_non_finite_norm_skips_the_optimizer_only(world, hip_device):
    """loss-scaled gradients with an inf norm: ssseg_sgd_step returns without touching anything; then, as in the
    separate sequence, the gradient is cleared and the EMA and both repacks run on the unchanged parameters"""
    amp = torch.tensor(E.amp_initial(), device=hip_device)
    want, got, _ = _run_both(world, 1.0, False, 5e-4, SGD | EMA | CLEAR, amp=amp, sq=float('inf'))
    _same(want, got, 'inf norm')
    init = world.initial[0]
    for k in ('p', 'buf'):
        E.same_bits(_bits(got[0][k]), _bits(init[k]), f'inf norm: {k} unchanged')
    assert not bool(got[0]['g'].any())
    h = {k: v.cpu().numpy() for k, v in init.items()}
    E.same_bits(got[0]['ema'].cpu().numpy(), E.ema_ref(h['ema'], h['p'], ALPHA), 'inf norm: ema')


def test_ema_without_an_optimizer_step(world):
    """SGD off, EMA on (a step that takes no optimizer step): only ema and the teacher's packs change"""
    want, got, _ = _run_both(world, 0.0, False, 5e-4, EMA)
    _same(want, got, 'ema only')
    init, packs0 = world.initial
    for k in ('p', 'g', 'buf'):
        E.same_bits(_bits(got[0][k]), _bits(init[k]), f'ema only: {k} unchanged')
    teacher = [t for _, _, _, shape, packs in world.slots if shape is not None for t, _ in packs]
    for i, (p, q, t) in enumerate(zip(got[1], packs0, teacher)):
        assert bool((p == -7.0).all()) == (not t), f'pack {i}'


def test_a_weight_stepped_twice_is_caught(world):
    """Each weight must be updated exactly once.  The comparison above notices a second update: the (72,40,3,3)
    weight's descriptor given again (as a second launch, so that the two updates cannot coincide) moves p, buf and
    ema away from the separate sequence's."""
    world.restore()
    world.separate(0.0, False, 5e-4, SGD | EMA | CLEAR)
    want = world.state()
    world.restore()
    world.fused(0.0, False, 5e-4, SGD | EMA | CLEAR)
    w3 = [w for w in world.weights if w[1] == (72, 40, 3, 3)]
    dup = world.table(w3)
    only_w3 = (dup[0][[i for i, d in enumerate(dup[0].tolist()) if d[2] != 0]].contiguous(), 1, dup[2])
    world.fused(0.0, False, 5e-4, SGD | EMA, plan=only_w3)
    got = world.state()
    torch.cuda.synchronize()
    assert _differs(want, got)
    with pytest.raises(AssertionError):
        _same(want, got, 'duplicate')


def test_two_captured_replays_equal_two_eager_steps(world):
    """the launch takes device pointers and a stream only: captured once, replayed twice = two eager steps"""
    g0 = world.initial[0]['g']
    max_norm = float(np.float32(0.25 * world.norm()))

    def one_step():
        world.t['g'].copy_(g0)          # the next backward's gradients
        world.fused(max_norm, False, 5e-4, SGD | EMA | CLEAR)

    world.restore()
    one_step()
    one_step()
    want = world.state()
    torch.cuda.synchronize()
    world.restore()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step()                      # warm-up on the capture stream's allocator
    torch.cuda.current_stream().wait_stream(side)
    world.restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step()
    world.restore()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    _same(want, world.state(), 'replay')


def _train(dev, steps=6, size=32, batch=2):
    """a few semi-supervised steps of a small SimpleUNet pair in the bf16 mode through train.train_step; returns the
    losses, both state dicts and how many fused launches ran (with and without an optimizer step)"""
    import cowmix
    import losses
    import train
    from models import simple_unet
    from models.adapters import ListOutput
    from ssseg import arena, optim, param_step
    cowmix._DEVICE_RNG['ctr'].clear()
    torch.manual_seed(0)
    student = ListOutput(simple_unet.UNet(2, 2, 8, 16)).to(dev)
    teacher = ListOutput(simple_unet.UNet(2, 2, 8, 16)).to(dev)
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.detach_()
    teacher.eval()
    arena.attach(student)
    arena.attach(teacher, with_grads=False)
    opt = optim.SGD(student.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    cfg = {'train': dict(
        loss=losses.CalculateLoss([{'loss_fn': losses.DenseBinaryCrossEntropyLossWithLogits('mean'), 'weight': [0.5]}]),
        virtual_batch_size_multiplier=1, use_semi_supervised=True, mask_proportion_range=(0.45, 0.55),
        sigma_range=(2, 4), consistency_loss_weight=10, ema_model_alpha=0.99, confidence_threshold=0.5,
        gradient_clip_value=5.0, print_freq=10 ** 9)}
    calls = []
    real = param_step.launch

    def counted(*a, **k):
        calls.append(a[12])     # flags
        return real(*a, **k)

    param_step.launch = counted
    try:
        g = torch.Generator().manual_seed(21)
        recs = []
        student.train()
        opt.zero_grad()
        for step in range(steps):
            img = torch.rand(batch, 3, size, size, generator=g).to(dev)
            fg = (torch.rand(batch, 1, size, size, generator=g) > 0.5).float()
            mask = torch.cat([1 - fg, fg], 1).to(dev)
            ua = torch.rand(batch, 3, size, size, generator=g).to(dev)
            ub = torch.rand(batch, 3, size, size, generator=g).to(dev)
            out = train.train_step(student, teacher, opt, img, mask, ua, ub, 30, step, cfg)
            recs.append(torch.stack([t.float() for t in out]).cpu())
        torch.cuda.synchronize()
    finally:
        param_step.launch = real
    state = {f'{n}.{k}': v.detach().float().cpu().clone() for n, m in (('s', student), ('t', teacher))
             for k, v in m.state_dict().items()}
    return torch.stack(recs), state, calls


def test_train_step_takes_the_fused_launch_and_computes_the_same(hip_device, monkeypatch):
    """train.train_step with the fused launch (taken as soon as both models' pack tables are built) and with
    SSSEG_PARAM_STEP=0: the same losses, parameters, momentum-driven updates, teacher and BN buffers, bit for bit"""
    monkeypatch.setenv('SSSEG_PARAM_STEP', '0')
    recs0, state0, calls0 = _train(hip_device)
    assert calls0 == []
    monkeypatch.delenv('SSSEG_PARAM_STEP')
    recs1, state1, calls1 = _train(hip_device)
    assert calls1.count(SGD | EMA | CLEAR) >= 2, calls1      # at least two of the five optimizer steps
    E.same_bits(recs1.numpy(), recs0.numpy(), 'losses')
    assert state0.keys() == state1.keys()
    for k in state0:
        E.same_bits(state1[k].numpy(), state0[k].numpy(), k)
