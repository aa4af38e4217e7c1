#!/usr/bin/env python3
"""tests/golden/mse.npz: the seeded inputs of tests/mse_ref.py CASES and what the REFERENCE's own MseLoss (losses/mse_loss.py,
imported live) computes for them on the CPU.

    python tools/make_mse_golden.py --reference /path/to/reference [--check]

The loss is built with MseLoss.__new__ + nn.Module.__init__ + cfg + a CPU Normal(0, 1) (its constructor moves the distribution
to a GPU); for the duration of a call Normal.sample hands out the recorded noise.  losses/mse_loss.py calls
matrix_vector_product, matrix_vector_product_T and BackwardSubst with four arguments (A, B, C, X) but leaves their import
commented out (:5): for the diag = false cases this tool binds the three names in the module's namespace to adapters over the
reference's own utils/triag_solve.py operators with D = 0 (the Python substitutions stand in for its absent CUDA extension,
as tools/make_triag_golden.py arranges).  utils/flow_utils.py imports cv2 at its top; where there is none an empty stand-in module
is registered (resize_flow does not use it).  Every case runs in float64 and in fp32.  Per case <c> of mse_ref.CASES (B = 2, level
6 x 10):
  net_<c>, target_<c>, eps_<c>      fp32 inputs: output[2] [2,8,6,10], the ground truth [2,2,H,W], the noise [S 2,2,6,10]
  total_, mse_, entropy_, offdiag_<c>, gnet_<c>   float64 run: the four outputs and d total / d net
  f32_<output>_<c>                  the outputs of the fp32 run
  noise_<output>_<c>, noise_gnet_<c>   max |fp32 run - float64 run| / max |float64 run| of the reference itself
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from arflow_amd.config import AttrDict  # noqa: E402
from tests import mse_ref as R  # noqa: E402
from make_triag_golden import reference_module  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'mse.npz')


def bind_missing_names(module, T):
    """The 4-argument call sites of losses/mse_loss.py:48,57,128 on the reference's 5-argument operators with a zero D."""
    def zero_d(A):
        return torch.zeros(A.shape[0], A.shape[1], A.shape[2] - 1, A.shape[3] - 1, dtype=A.dtype)
    module.matrix_vector_product = lambda A, B, C, X: T.matrix_vector_product(A, B, C, zero_d(A), X)
    module.matrix_vector_product_T = lambda A, B, C, X: T.matrix_vector_product_T(A, B, C, zero_d(A), X)
    module.BackwardSubst = types.SimpleNamespace(apply=lambda A, B, C, X: T.BackwardSubst.apply(A, B, C, zero_d(A), X))


def run_case(module, tag, inp, dtype):
    cfg = AttrDict(R.case_cfg(tag))
    loss = module.MseLoss.__new__(module.MseLoss)
    torch.nn.Module.__init__(loss)
    loss.cfg = cfg
    loss.Normal = torch.distributions.Normal(0, 1)
    net = torch.from_numpy(inp['net']).to(dtype).requires_grad_(True)
    queue = [torch.from_numpy(inp['eps']).to(dtype)]
    Normal = torch.distributions.Normal
    saved = Normal.sample

    def sample(self, size=torch.Size()):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(size), (tuple(t.shape), tuple(size))
        return t
    Normal.sample = sample
    try:
        res = loss([None, None, net], torch.from_numpy(inp['target']).to(dtype))
    finally:
        Normal.sample = saved
    assert not queue
    (g,) = torch.autograd.grad(res[0], net)
    out = {k: np.asarray(torch.as_tensor(v).detach().to(dtype).numpy()) for k, v in zip(R.OUTPUTS, res)}
    out['gnet'] = g.numpy()
    return out


def generate(reference_root):
    if 'easydict' not in sys.modules:
        mod = types.ModuleType('easydict')
        mod.EasyDict = AttrDict
        sys.modules['easydict'] = mod
    if 'cv2' not in sys.modules:  # utils/flow_utils.py imports it at its top; resize_flow does not use it
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.modules['cv2'] = types.ModuleType('cv2')
    T = reference_module(reference_root)
    import losses.mse_loss as L
    bind_missing_names(L, T)
    out = {}
    for tag in R.CASES:
        inp = R.make_inputs(tag)
        r64, r32 = run_case(L, tag, inp, torch.float64), run_case(L, tag, inp, torch.float32)
        for k, v in inp.items():
            out['%s_%s' % (k, tag)] = v
        for k, v in r64.items():
            out['%s_%s' % (k, tag)] = v.astype(np.float64)
            scale = np.abs(v).max()
            gap = np.abs(r32[k].astype(np.float64) - v).max()
            out['noise_%s_%s' % (k, tag)] = np.float64(gap / scale if scale > 0 else gap)
            if k != 'gnet':
                out['f32_%s_%s' % (k, tag)] = r32[k].astype(np.float32)
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
            print('  %-24s %.3e' % (k, out[k]))


if __name__ == '__main__':
    main()
