#!/usr/bin/env python3
"""tests/golden/elbo.npz: seeded inputs (tests/elbo_ref.py) and what the REFERENCE's own code (losses/uflow_elbo_loss.py and
utils/triag_solve.py, imported live) computes for them.

    python tools/make_elbo_golden.py --reference /path/to/reference [--check]

The loss draws its noise from `self.Normal.sample(size)`; this tool replaces that object by one that hands out the recorded
noise of the case in the order the loss asks for it (forward direction first), so the reference runs its own code on known
samples.  Every case runs twice, in float64 and in fp32.

Per loss case (tests/elbo_ref.py CASES; B = 2, 32 x 64 images, an 8 x 16 level 2):
  net12_, net21_, eps12_, eps21_<case>   the fp32 inputs and the noise (the images im1, im2 are shared by all cases)
  <output>_<case>                        the float64 run: total, warp, smooth, entropy, oof, flow12_2, occu_mask12,
                                         valid_mask12, and gnet12, gnet21 = the gradients of total w.r.t. both level-2 outputs
  noise_<output>_<case>                  max |fp32 run - float64 run| / max |float64 run| of the reference itself
Per banded-operator case mv_<grid>_k<k> / mvT_<grid>_k<k> (inputs: elbo_ref.make_band_case(2, 1, M, N, k), not stored;
`insum_*` is the float64 sum of all of them, against a drift of the recipe): Y_, gX_, gA_ of sum(gY * Y) in float64 for the
grids the reference's slicing can run (it needs M, N >= k); the three larger test grids hold Y_ and gX_ at k = 3 only.
--check regenerates in memory and compares with the committed file instead of writing it.  The file holds arrays only.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import elbo_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'elbo.npz')


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


def run_product(fn, case, k, dtype):
    A = torch.from_numpy(np.concatenate((case['diag'], case['off']), 1)).to(dtype).requires_grad_(True)
    X = torch.from_numpy(case['X']).to(dtype).requires_grad_(True)
    Y = fn(A, X, k=k)
    Y.backward(torch.from_numpy(case['gY']).to(dtype))
    return {'Y': Y.detach().numpy(), 'gX': X.grad.numpy(), 'gA': A.grad.numpy()}


def generate(reference_root):
    sys.path.insert(0, reference_root)
    import losses.uflow_elbo_loss as L
    import utils.triag_solve as T
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
    jobs = [(tag, k, ('Y', 'gX', 'gA')) for tag, ks in R.GOLDEN_GRIDS.items() for k in ks]
    jobs += [(tag, 3, ('Y', 'gX')) for tag in R.GOLDEN_BIG]
    for tag, k, keep in jobs:
        M, N = R.grid_shape(tag)
        case = R.make_band_case(2, 1, M, N, k)
        for name, fn in (('mv', T.matrix_vector_product_general), ('mvT', T.matrix_vector_product_T_general)):
            r = run_product(fn, case, k, torch.float64)
            for key in keep:
                out['%s_%s_%s_k%d' % (key, name, tag, k)] = r[key]
        out['insum_%s_k%d' % (tag, k)] = np.float64(sum(v.astype(np.float64).sum() for v in case.values()))
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
