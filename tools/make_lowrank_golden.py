#!/usr/bin/env python3
"""tests/golden/elbo_lowrank.npz: seeded inputs (tests/lowrank_ref.py) and what the REFERENCE's own code (losses/
uflow_elbo_loss.py and models/uflow_prob_model.py, imported live) computes for them with approx: 'lowrank'.

    python tools/make_lowrank_golden.py --reference /path/to/reference [--check]

As tools/make_elbo_golden.py, the loss's `self.Normal` is replaced by an object that hands out the recorded noise of the case
in the order the loss asks for it (forward direction first).  Every loss case runs twice, in float64 and in fp32.

Per loss case (tests/lowrank_ref.py CASES; B = 2, 32 x 64 images, an 8 x 16 level 2):
  net12_, net21_, eps12_, eps21_<case>   the fp32 inputs and the noise [S B,2R,1,1] (the images im1, im2 are shared)
  <output>_<case>                        the float64 run: total, warp, smooth, entropy, oof, flow12_2, occu_mask12,
                                         valid_mask12, and gnet12, gnet21 = the gradients of total w.r.t. both level-2 outputs
  noise_<output>_<case>                  max |fp32 run - float64 run| / max |float64 run| of the reference itself
Per model case (MODEL_CASES: out_channels [2,0,30] and [2,0,6]; input, weights and pooling of tools/make_prob_golden.py):
  keys_<case>, params_<case>             the state_dict's key order and the parameter count
  out_<case>_<fw|bw>_<level>             the stored channels (lowrank_ref.stored_channels) of that output
  insum                                  float64 sum of the model's input pair, against a drift of the recipe
--check regenerates in memory and compares with the committed file instead of writing it.  The file holds arrays only.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from arflow_amd.config import AttrDict  # noqa: E402
from tests import lowrank_ref as R  # noqa: E402
from tests import prob_ref as P  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'elbo_lowrank.npz')


class Recorded:
    """Stands in for torch.distributions.Normal(0, 1): sample(size) returns the next recorded tensor."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def sample(self, size):
        t = self.tensors.pop(0)
        assert tuple(t.shape) == tuple(size), (tuple(t.shape), tuple(size))
        return t


def run_loss(module, tag, case, dtype):
    cfg = R.case_cfg(tag)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in case.items()}
    net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
    loss = module.UFlowElboLoss(cfg)
    loss.Normal = Recorded([t['eps12'], t['eps21']])
    res = loss({'flows_fw': [None, None, net12], 'flows_bw': [None, None, net21]}, t['im1'], t['im2'])
    res[0].backward()
    out = dict(zip(R.OUTPUTS[:8], res))
    out.update(gnet12=net12.grad, gnet21=net21.grad)
    return {k: torch.as_tensor(v, dtype=dtype).detach().numpy() for k, v in out.items()}


def generate(reference_root):
    if 'easydict' not in sys.modules:
        mod = types.ModuleType('easydict')
        mod.EasyDict = AttrDict
        sys.modules['easydict'] = mod
    sys.path.insert(0, reference_root)
    import losses.uflow_elbo_loss as L
    import models.uflow_prob_model as M
    out = {}
    shared = R.make_loss_case(sorted(R.CASES)[0])
    out['im1'], out['im2'] = shared['im1'], shared['im2']
    for tag in R.CASES:
        case = R.make_loss_case(tag)
        for k in ('net12', 'net21', 'eps12', 'eps21'):
            out['%s_%s' % (k, tag)] = case[k]
        r64, r32 = run_loss(L, tag, case, torch.float64), run_loss(L, tag, case, torch.float32)
        for k, v in r64.items():
            out['%s_%s' % (k, tag)] = v
            scale = np.abs(v).max()
            gap = np.abs(r32[k].astype(np.float64) - v).max()
            out['noise_%s_%s' % (k, tag)] = np.float64(gap / scale if scale > 0 else gap)
    img1, img2, insum = P.make_input()
    out['insum'] = np.float64(insum)
    torch.set_num_threads(8)
    for tag in R.MODEL_CASES:
        model = R.prepare(M.PWCProbFlow(R.model_cfg(tag)))
        out['keys_' + tag] = np.array(list(model.state_dict().keys()))
        out['params_' + tag] = np.int64(sum(p.numel() for p in model.parameters()))
        with torch.no_grad():
            res = model(img1, img2, with_bk=True)
        assert len(res['flows_fw']) == 6 and len(res['flows_bw']) == 6
        out.update(R.collect(res, tag))
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
    print('%s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))
    for k in sorted(out):
        if k.startswith('noise_'):
            print('  %-40s %.3e' % (k, out[k]))


if __name__ == '__main__':
    main()
