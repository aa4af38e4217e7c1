"""losses/get_loss.py:9-24: every loss type of the reference -- 'unflow', 'elbo', 'fullres', 'uflow', 'uflow_elbo' and the
supervised 'mse' (DESIGN.md sections 21, 27 and 28) -- and the build-defined 'mv'."""
from .elbo_loss import ElboLoss
from .flow_loss import unFlowLoss
from .fullres_loss import FullResLoss
from .mse_loss import MseLoss
from .mv_loss import MvLoss
from .uflow_elbo_loss import UFlowElboLoss, UFlowElboPenLoss, takes_default_path
from .uflow_loss import UFlowLoss


def get_loss(cfg):
    if cfg.type == 'unflow':
        return unFlowLoss(cfg)
    if cfg.type == 'elbo':
        return ElboLoss(cfg)
    if cfg.type == 'fullres':
        return FullResLoss(cfg)
    if cfg.type == 'uflow':
        return UFlowLoss(cfg)
    if cfg.type == 'uflow_elbo':
        # selectable penalties / mean-flow masks: the subclass on the penalised kernels
        return UFlowElboLoss(cfg) if takes_default_path(cfg) else UFlowElboPenLoss(cfg)
    if cfg.type == 'mse':
        return MseLoss(cfg)
    if cfg.type == 'mv':  # build-defined 3-frame objective; not a reference type
        return MvLoss(cfg)
    raise NotImplementedError(cfg.type)
