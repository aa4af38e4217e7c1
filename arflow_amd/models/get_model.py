"""models/get_model.py:8-25: the deterministic flow models and PWCProbFlow, the single-pyramid probabilistic model of
configs/chairs_uflow_elbo*.json, and ComponentNet, the two-pyramid model of the mixture family (DESIGN.md section 26;
MixtureWeightsNet and PWCLiteProb are out of scope)."""
from .pwclite import PWCLite
from .pwclite_uflow import PWCLiteUflow
from .uflow_model import PWCFlow
from .uflow_prob_model import ComponentNet, PWCProbFlow


def get_model(cfg):
    if cfg.type == 'pwclite':
        return PWCLite(cfg)
    if cfg.type == 'pwclite_uflow':
        return PWCLiteUflow(cfg)
    if cfg.type == 'uflow':
        return PWCFlow(cfg)
    if cfg.type == 'uflow_prob':
        return PWCProbFlow(cfg)
    if cfg.type == 'component':
        return ComponentNet(cfg)
    raise NotImplementedError(cfg.type)
