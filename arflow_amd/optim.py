"""The `train` section of a config as one fused optimiser step on the native kernels of csrc/optim.hip.

The reference builds its optimiser in trainer/base_trainer.py:78-129 -- two parameter groups (decayed weights, undecayed biases
and BatchNorm weights), then torch.optim.Adam, its own AdamW (utils/torch_utils.py:82-161: decoupled decay NOT scaled by lr,
eps outside the bias correction) or torch.optim.SGD with momentum -- clips the global gradient norm in front of the step
(trainer/uflow_elbo_trainer.py:94-99) and decays lr by ExponentialLR once an epoch from lr_decay_start_epoch on
(base_trainer.py:52-54).  FlatOptimizer does the same on the flat gradient buffer of ddp.FlatGradAllReduce: the state lives in flat
buffers of the gradient's layout and ONE launch steps every parameter of the model; with clipping (or the non-finite guard) one
launch in front of it stores the partial sums of the squared gradient norm.  Nothing is read back: a step enqueues and returns.

Stated differences from the reference:
  * the clip multiplies the gradient as the step READS it; ``param.grad`` keeps the unclipped values (nobody reads .grad
    between the clip and the next zero_grad);
  * EVERY parameter is stepped EVERY step: a parameter that received no gradient has a zero gradient in the flat buffer (as
    with TrainStep's torch.optim.Adam over the same buffer), where the reference skips a parameter whose .grad is None.  With
    a zero gradient Adam still moves the parameter by its decaying first moment, and L2 decay still applies;
  * with skip_nonfinite the step count advances on the host also for a step the device skipped (the host reads nothing).

GPU only: a CPU tensor raises ArflowHipError.
"""
import math

import numpy as np
import torch

from . import _lib
from .functional import _call, _p, _stream

__all__ = ['decay_groups', 'chunk_table', 'FlatOptimizer', 'CHUNK', 'RULES']

CHUNK = 2048  # ARFLOW_OPTIM_CHUNK of include/arflow_hip.h
ROW = 4       # ARFLOW_OPTIM_ROW: address, flat offset, count, weight decay (the bits of a double)
RULES = {'adam': 0, 'adamw': 1, 'sgd': 2}


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        v = cfg.get(key, default)
    else:
        v = getattr(cfg, key, default)
    return default if v is None else v


def decay_groups(model, weight_decay, bias_decay):
    """The two groups of trainer/base_trainer.py:81-112 -> [{'names', 'params', 'weight_decay'}] (decay, no decay), each sorted
    by full parameter name: a name ending in `bias` is not decayed, `weight` of Conv2d / ConvTranspose2d / Linear is,
    BatchNorm2d.weight is not.  A parameter in neither set raises with the reference's message."""
    decay, no_decay = set(), set()
    whitelist = (torch.nn.Linear, torch.nn.Conv2d, torch.nn.ConvTranspose2d)
    blacklist = (torch.nn.BatchNorm2d,)
    for mn, m in model.named_modules():
        for pn, _ in m.named_parameters():
            fpn = '%s.%s' % (mn, pn) if mn else pn
            if pn.endswith('bias'):
                no_decay.add(fpn)
            elif pn.endswith('weight') and isinstance(m, whitelist):
                decay.add(fpn)
            elif pn.endswith('weight') and isinstance(m, blacklist):
                no_decay.add(fpn)
    params = dict(model.named_parameters())
    both, rest = decay & no_decay, params.keys() - (decay | no_decay)
    assert len(both) == 0, 'parameters %s made it into both decay/no_decay sets!' % (str(both),)
    assert len(rest) == 0, 'parameters %s were not separated into either decay/no_decay set!' % (str(rest),)
    return [dict(names=sorted(decay), params=[params[n] for n in sorted(decay)], weight_decay=weight_decay),
            dict(names=sorted(no_decay), params=[params[n] for n in sorted(no_decay)], weight_decay=bias_decay)]


def chunk_table(spans, chunk=CHUNK):
    """spans: (address, flat offset, count, weight decay) per parameter tensor -> int64 [rows, 4], the device table's layout:
    every tensor cut into rows of at most `chunk` elements, no row crossing a tensor.  Pure host."""
    rows = []
    for addr, off, n, wd in spans:
        bits = int(np.float64(wd).view(np.int64))
        for s in range(0, int(n), chunk):
            rows.append((int(addr) + 4 * s, int(off) + s, min(chunk, int(n) - s), bits))
    return np.asarray(rows, dtype=np.int64).reshape(-1, ROW)


class FlatOptimizer:
    """``FlatOptimizer(reducer, cfg)``: reducer is the model's ddp.FlatGradAllReduce, cfg the `train` section of a config (an
    AttrDict or dict): optim ('adam': lr, beta1, beta2, eps | 'adamw': lr, betas (momentum, beta), eps 1e-8 | 'sgd': lr,
    momentum), weight_decay, bias_decay, clip (<= 0 or missing: off), lr_decay_factor, lr_decay_start_epoch, skip_nonfinite
    (default False: with it a step whose gradient norm is not finite writes nothing but the device counter `skipped`).
    Call step() after reducer.finish(); every rank then takes the identical step."""

    def __init__(self, reducer, cfg):
        self.optim = _get(cfg, 'optim')
        if self.optim not in RULES:
            raise NotImplementedError(self.optim)
        self.reducer = reducer
        flat = reducer.flat
        if not flat.is_cuda:
            raise _lib.ArflowHipError('arflow_amd.optim runs on the GPU only (the gradient buffer is a %s tensor); there is no '
                                      'CPU fallback' % flat.device)
        if flat.dtype != torch.float32:
            raise _lib.ArflowHipError('arflow_amd.optim is fp32 only (got %s)' % flat.dtype)
        self.lr = float(_get(cfg, 'lr'))
        if self.optim == 'adam':
            self.betas, self.eps = (float(_get(cfg, 'beta1')), float(_get(cfg, 'beta2'))), float(_get(cfg, 'eps'))
        elif self.optim == 'adamw':
            self.betas, self.eps = (float(_get(cfg, 'momentum')), float(_get(cfg, 'beta'))), 1e-8
        else:
            self.betas, self.eps = (float(_get(cfg, 'momentum')), 0.0), 0.0
        self.clip = float(_get(cfg, 'clip', -1.0))
        self.lr_decay_factor = float(_get(cfg, 'lr_decay_factor', 1.0))
        self.lr_decay_start_epoch = _get(cfg, 'lr_decay_start_epoch', float('inf'))
        self.skip_nonfinite = bool(_get(cfg, 'skip_nonfinite', False))
        groups = decay_groups(reducer.module, float(_get(cfg, 'weight_decay', 0.0)), float(_get(cfg, 'bias_decay', 0.0)))
        self._decay = {id(p): g['weight_decay'] for g in groups for p in g['params']}
        self.t = 0
        self.exp_avg = torch.zeros_like(flat)  # momentum_buffer for sgd
        self.exp_avg_sq = torch.zeros_like(flat) if self.optim != 'sgd' else None
        self.skipped = torch.zeros(1, device=flat.device, dtype=torch.int32)
        lib = _lib.load()
        self._nparts = lib.arflow_optim_partials(flat.numel())
        _lib.check(min(self._nparts, 0), 'arflow_optim_partials')
        self._partials = torch.empty(self._nparts, device=flat.device, dtype=torch.float64)
        self._ptrs, self._table = None, None

    momentum_buffer = property(lambda self: self.exp_avg)

    def _current_ptrs(self):
        return [p.data_ptr() for p, _, _ in self.reducer._spans]

    def _build_table(self, ptrs):
        flat = self.reducer.flat
        for p, _, _ in self.reducer._spans:
            if not p.is_cuda or p.device != flat.device:
                raise _lib.ArflowHipError('arflow_amd.optim runs on the GPU only (a parameter is on %s, the gradient buffer on '
                                          '%s); there is no CPU fallback' % (p.device, flat.device))
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.ArflowHipError('arflow_amd.optim needs contiguous fp32 parameters (got %s, strides %s)'
                                          % (p.dtype, p.stride()))
        host = chunk_table([(a, o, n, self._decay[id(p)]) for a, (p, o, n) in zip(ptrs, self.reducer._spans)])
        self._table = torch.from_numpy(host).to(flat.device)
        self._ptrs = ptrs

    def step(self):
        """One step from the gradient in the reducer's flat buffer, on the current stream; no synchronisation, nothing read."""
        flat = self.reducer.flat
        ptrs = self._current_ptrs()
        if ptrs != self._ptrs:  # a parameter's storage moved (p.data = ..., .to()): a stale row must never become an address
            self._build_table(ptrs)
        self.t += 1
        b1, b2 = self.betas
        bc1 = 1.0 - b1 ** self.t if self.optim != 'sgd' else 1.0
        sqbc2 = math.sqrt(1.0 - b2 ** self.t) if self.optim != 'sgd' else 1.0
        clip = self.clip if self.clip > 0 else -1.0
        norm = clip > 0 or self.skip_nonfinite
        n = flat.numel()
        with torch.cuda.device_of(flat):
            if norm:
                _call('arflow_optim_gradnorm', _p(flat), _p(self._partials), n, _stream(), key=(n,))
            _call('arflow_optim_step', _p(self._table), int(self._table.shape[0]), _p(flat), _p(self.exp_avg), _p(self.exp_avg_sq),
                  n, _p(self._partials) if norm else None, self._nparts if norm else 0,
                  _p(self.skipped) if self.skip_nonfinite else None, RULES[self.optim], int(self.t == 1), self.lr, bc1, sqbc2,
                  self.eps, b1, b2, clip, _stream(), key=(n, self.optim, int(norm)))

    def zero_grad(self):
        self.reducer.zero_grad()

    def epoch_end(self, i_epoch):
        """base_trainer.py:52-54 with ExponentialLR: lr *= lr_decay_factor once i_epoch >= lr_decay_start_epoch."""
        if i_epoch >= self.lr_decay_start_epoch:
            self.lr = self.lr * self.lr_decay_factor
        return self.lr

    def skipped_steps(self):
        """The device counter of the non-finite guard (synchronises)."""
        return int(self.skipped.item())

    def state_dict(self):
        return {'optim': self.optim, 'step': self.t, 'lr': self.lr, 'exp_avg': self.exp_avg.clone(),
                'exp_avg_sq': None if self.exp_avg_sq is None else self.exp_avg_sq.clone(), 'skipped': self.skipped.clone()}

    def load_state_dict(self, state):
        if state['optim'] != self.optim:
            raise ValueError('the state is of optim %r, this optimiser is %r' % (state['optim'], self.optim))
        if tuple(state['exp_avg'].shape) != tuple(self.exp_avg.shape):
            raise ValueError('the state holds %d elements, the model has %d' % (state['exp_avg'].numel(), self.exp_avg.numel()))
        self.t, self.lr = int(state['step']), float(state['lr'])
        self.exp_avg.copy_(state['exp_avg'])
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.copy_(state['exp_avg_sq'])
        self.skipped.copy_(state['skipped'])
