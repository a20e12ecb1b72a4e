"""diffGrad (arXiv:1909.11015), fused over the flat arena."""
from ssseg import native as N
from ssseg.optim import FusedOptimizer, _check_adam_family


class DiffGrad(FusedOptimizer):
    """Adam whose first moment is damped by a friction coefficient computed from the change of the gradient since the
    previous step (version 0: sigmoid(|d|), 1: sigmoid(d), 2: 9 * sigmoid(|d| / 2) - 4).  previous_grad holds the
    previous step's gradient, weight-decay term included."""
    MODE = N.OPT_DIFFGRAD
    STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'previous_grad')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, version=0, weight_decay=0):
        _check_adam_family(lr, eps, betas)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.version = version
