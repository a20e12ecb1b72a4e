"""Ranger = RAdam (arXiv:1908.03265) + Lookahead (arXiv:1907.08610), fused over the flat arena."""
from ssseg import native as N
from ssseg.optim import FusedOptimizer


class Ranger(FusedOptimizer):
    """Rectified Adam whose parameters are pulled towards a slow copy every k steps (slow += alpha * (p - slow);
    p = slow).  While the approximated SMA length N_sma is at most N_sma_threshhold the step is plain bias-corrected
    momentum, afterwards the rectified adaptive step.  The slow copy starts from the parameters as they stand on
    entry to the first step (not at construction: a checkpoint may be loaded in between)."""
    MODE = N.OPT_RANGER
    STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'slow_buffer')

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5,
                 weight_decay=0):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not lr > 0:
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        super().__init__(params, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas,
                                      N_sma_threshhold=N_sma_threshhold, eps=eps, weight_decay=weight_decay))
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k

    def _hyper(self, g):
        # like the reference: k per group, alpha and the threshold from the optimizer's attributes
        return 0.0, g['k'], self.N_sma_threshhold, self.alpha
