"""losses/get_loss.py:9-24 for the loss types on the hot path and the ELBO objectives of the probabilistic families (DESIGN.md
sections 21 and 27; the MSE research losses are out of scope)."""
from .elbo_loss import ElboLoss
from .flow_loss import unFlowLoss
from .fullres_loss import FullResLoss
from .mv_loss import MvLoss
from .uflow_elbo_loss import UFlowElboLoss
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
        return UFlowElboLoss(cfg)
    if cfg.type == 'mv':  # build-defined 3-frame objective; not a reference type
        return MvLoss(cfg)
    raise NotImplementedError(cfg.type)
