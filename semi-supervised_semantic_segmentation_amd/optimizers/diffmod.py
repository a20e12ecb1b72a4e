"""DiffMod = diffGrad's friction coefficient on AdaMod's bounded step, fused over the flat arena."""
from ssseg import native as N
from ssseg.optim import FusedOptimizer, _check_adam_family


class DiffMod(FusedOptimizer):
    """AdaMod (decoupled weight decay, learning rates bounded by their moving average) with the first moment damped
    by diffGrad's friction coefficient.  len_memory is AdaMod's beta3 in an easier form: beta3 = 1 - 1/len_memory."""
    MODE = N.OPT_DIFFMOD
    STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'exp_avg_lr', 'previous_grad')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), len_memory=1000, version=0, eps=1e-8, weight_decay=0):
        _check_adam_family(lr, eps, betas)
        beta3 = 1 - (1 / len_memory)
        if not 0.0 <= beta3 < 1.0:
            raise ValueError("Invalid beta3 parameter: {}".format(beta3))
        super().__init__(params, dict(lr=lr, betas=betas, beta3=beta3, eps=eps, weight_decay=weight_decay))
        self.version = version
