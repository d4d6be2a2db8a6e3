from .fused_sgd import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, Lookahead  # noqa: F401
from . import lr_scheduler  # noqa: F401
