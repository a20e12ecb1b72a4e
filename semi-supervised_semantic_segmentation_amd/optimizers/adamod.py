"""AdaMod (arXiv:1910.12249) with decoupled weight decay, fused over the flat arena."""
from ssseg import native as N
from ssseg.optim import FusedOptimizer, _check_adam_family


class AdaMod(FusedOptimizer):
    """Adam whose per-element learning rates are bounded from above by their own exponential moving average
    (exp_avg_lr, smoothing beta3)."""
    MODE = N.OPT_ADAMOD
    STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'exp_avg_lr')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), beta3=0.999, eps=1e-8, weight_decay=0):
        _check_adam_family(lr, eps, betas)
        if not 0.0 <= beta3 < 1.0:
            raise ValueError("Invalid beta3 parameter: {}".format(beta3))
        super().__init__(params, dict(lr=lr, betas=betas, beta3=beta3, eps=eps, weight_decay=weight_decay))
