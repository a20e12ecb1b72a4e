"""The reference's `optimizers` package (Ranger, AdaMod, DiffGrad, DiffMod) on the fused device step.

Same import paths, constructor signatures, defaults and ValueError checks as the reference's classes, so a reference
config (`from optimizers.ranger import Ranger`) imports and runs unchanged; the update itself is
ssseg.optim.FusedOptimizer: two launches over the flat parameter arena.  Importing needs no GPU.
"""
from .adamod import AdaMod
from .diffgrad import DiffGrad
from .diffmod import DiffMod
from .ranger import Ranger

__all__ = ['Ranger', 'AdaMod', 'DiffGrad', 'DiffMod']
