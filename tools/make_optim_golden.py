#!/usr/bin/env python3
"""tests/golden/optim.npz: the seeded inputs of tests/optim_ref.py and what torch's own optimisers, the REFERENCE's AdamW
(utils/torch_utils.py, imported live: it runs on this torch with a deprecation warning) and the reference's
BaseTrainer._create_optimizer (trainer/base_trainer.py, imported live) make of them, on the CPU in float64.

    python tools/make_optim_golden.py --reference /path/to/reference [--check]

trainer/base_trainer.py imports tensorboardX at its top; where there is none an empty stand-in module with a SummaryWriter name is
registered (nothing here constructs a trainer: _create_optimizer is called unbound on a namespace holding model, cfg and a log).
  sizes, names            the parameter set of optim_ref (1-D tensors, alternately `weight` of a Linear and `bias`)
  p0 [N], g [3, N]        fp32 parameters and the three recorded gradient sets, in the order of `names`
  idx                     the elements whose trajectories are recorded: every element of the five small tensors, and of the three
                          long ones the first, the last and every 61st (the rules are elementwise; the norm reads all of g)
  clip_on, clip_slack     the two clip values (a quarter of the smallest gradient norm, four times the largest)
  p_<case>, m_<case>, v_<case> [3, len(idx)]   float64 parameters and state after each of three steps; case = rule_clip of
                          optim_ref.CASES: torch.optim.Adam without / with decay, the reference's AdamW, torch.optim.SGD (m is
                          its momentum_buffer, no v), each with clip_grad_norm_ active, slack and absent
  lr_schedule             the lr after each of the epochs optim_ref.SCHEDULE names, ExponentialLR stepped as base_trainer.py:52-54
  decay_<workload>, no_decay_<workload>   the names of the two groups _create_optimizer forms for the model of every workload of
                          arflow_amd.train_step.WORKLOADS, in group order
--check regenerates in memory and compares with the committed file instead of writing it.  Arrays and name lists only.
"""
import argparse
import logging
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from arflow_amd.config import AttrDict  # noqa: E402
from tests import optim_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'optim.npz')


def recorded_indices():
    idx, off = [], 0
    for n in R.SIZES:
        idx += list(range(off, off + n)) if n <= 16 else sorted(set(range(off, off + n, 61)) | {off + n - 1})
        off += n
    return np.asarray(idx, dtype=np.int64)


def reference_modules(reference_root):
    sys.path.insert(0, reference_root)
    if 'tensorboardX' not in sys.modules:
        try:
            import tensorboardX  # noqa: F401
        except ImportError:
            mod = types.ModuleType('tensorboardX')
            mod.SummaryWriter = object
            sys.modules['tensorboardX'] = mod
    import trainer.base_trainer as B
    import utils.torch_utils as T
    assert os.path.abspath(B.__file__).startswith(reference_root) and os.path.abspath(T.__file__).startswith(reference_root)
    return B, T


def split(flat):
    out, off = [], 0
    for n in R.SIZES:
        out.append(flat[off:off + n])
        off += n
    return out


def make_optimizer(B, T, cfg, params):
    """The branch of _create_optimizer a cfg takes, over the fixture's two groups (weights, biases)."""
    groups = [{'params': [p for n, p in zip(R.NAMES, params) if n.endswith('weight')], 'weight_decay': cfg.weight_decay},
              {'params': [p for n, p in zip(R.NAMES, params) if n.endswith('bias')], 'weight_decay': cfg.bias_decay}]
    if cfg.optim == 'adamw':
        return T.AdamW(groups, cfg.lr, betas=(cfg.momentum, cfg.beta))
    if cfg.optim == 'adam':
        return torch.optim.Adam(groups, cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    return torch.optim.SGD(groups, cfg.lr, momentum=cfg.momentum)


def run_case(B, T, case, p0, g, idx):
    cfg = AttrDict(R.case_cfg(case, g))
    params = [torch.nn.Parameter(torch.from_numpy(t.astype(np.float64))) for t in split(p0)]
    opt = make_optimizer(B, T, cfg, params)
    rec = {'p': [], 'm': [], 'v': []}
    for t in range(R.STEPS):
        for p, gt in zip(params, split(g[t])):
            p.grad = torch.from_numpy(gt.astype(np.float64))
        if cfg.clip > 0:
            torch.nn.utils.clip_grad_norm_(params, cfg.clip)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            opt.step()
        rec['p'].append(torch.cat([p.detach() for p in params]).numpy()[idx])
        if cfg.optim == 'sgd':
            rec['m'].append(torch.cat([opt.state[p]['momentum_buffer'] for p in params]).numpy()[idx])
        else:
            rec['m'].append(torch.cat([opt.state[p]['exp_avg'] for p in params]).numpy()[idx])
            rec['v'].append(torch.cat([opt.state[p]['exp_avg_sq'] for p in params]).numpy()[idx])
    return {k: np.stack(v) for k, v in rec.items() if v}


def lr_schedule(B):
    s = R.SCHEDULE
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], s['lr'])
    fake = types.SimpleNamespace(optimizer=opt, cfg=AttrDict(lr_decay_factor=s['lr_decay_factor']))
    sched = B.BaseTrainer._create_lr_scheduler(fake)
    out = []
    for i_epoch in s['epochs']:
        if i_epoch >= s['lr_decay_start_epoch']:
            opt.step()
            sched.step()
        out.append(sched.get_last_lr()[0])
    return np.asarray(out, dtype=np.float64)


def group_names(B):
    from arflow_amd.models import get_model
    from arflow_amd.train_step import WORKLOADS
    out = {}
    for name, (mcfg, _) in WORKLOADS.items():
        model = get_model(AttrDict(mcfg))
        fake = types.SimpleNamespace(_log=logging.getLogger('make_optim_golden'), model=types.SimpleNamespace(module=model),
                                     cfg=AttrDict(optim='sgd', lr=0.1, momentum=0.9, weight_decay=1e-6, bias_decay=0.0))
        opt = B.BaseTrainer._create_optimizer(fake)
        by_id = {id(p): n for n, p in model.named_parameters()}
        for key, grp in zip(('decay', 'no_decay'), opt.param_groups):
            out['%s_%s' % (key, name)] = np.asarray([by_id[id(p)] for p in grp['params']], dtype=np.str_)
    return out


def generate(reference_root):
    B, T = reference_modules(reference_root)
    p0, g = R.make_inputs()
    idx = recorded_indices()
    clips = R.clip_values(g)
    out = {'sizes': np.asarray(R.SIZES, dtype=np.int64), 'names': np.asarray(R.NAMES, dtype=np.str_), 'p0': p0, 'g': g, 'idx': idx,
           'clip_on': np.float64(clips['on']), 'clip_slack': np.float64(clips['slack']), 'lr_schedule': lr_schedule(B)}
    for case in R.CASES:
        for k, v in run_case(B, T, case, p0, g, idx).items():
            out['%s_%s' % (k, case)] = v
    out.update(group_names(B))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ARFLOW_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--check', action='store_true', help='compare with the committed file, write nothing')
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('give --reference (or set ARFLOW_REFERENCE)')
    out = generate(os.path.abspath(args.reference))
    if args.check:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for k, v in out.items():
            assert old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v), k
        print('%s reproduced: %d arrays equal' % (os.path.relpath(OUT, ROOT), len(out)))
        return
    np.savez_compressed(OUT, **out)
    print('%s: %d bytes, %d arrays, %d recorded elements of %d' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT), len(out),
                                                                   len(out['idx']), R.N))


if __name__ == '__main__':
    main()
