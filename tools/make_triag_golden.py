#!/usr/bin/env python3
"""tests/golden/triag.npz: seeded inputs (tests/triag_ref.py make_case) and what the REFERENCE's own code
(utils/triag_solve.py, imported live) computes for them.

    python tools/make_triag_golden.py --reference /path/to/reference [--check]

utils/triag_solve.py calls a global `triag_solve_cuda` that it never imports (its import line is commented out).  This
tool sets utils.triag_solve.triag_solve_cuda to a namespace whose forward_substitution and backward_substitution are the
reference's own Python functions of the same module (:76-115); a call with four arguments -- the stale signature of
marginal_variances, :214 -- gets a zero D.  With that in place ForwardSubst.apply, BackwardSubst.apply and
marginal_variances run the reference's code and nothing else.  (marginal_variances_fast fails with a shape error at :263
and is not used.)

Per solve case (tests/triag_ref.py SOLVE_CASES; `lo` = ForwardSubst, `up` = BackwardSubst, all with D):
  A_, B_, C_, D_, X_, gY_<case>      the fp32 inputs
  Y_, gX_, gA_, gB_, gC_, gD_<dir>_<case>   the float64 run: the solution and the gradients of sum(gY * Y)
  noise_<output>_<dir>_<case>        max |fp32 run - float64 run| / max |float64 run| of the reference itself
Per marginal-variance case (DIAG_CASES): A_, B_, C_diag_<case>, H_diag_<case> (float64) and noise_H_diag_<case>, the
largest RELATIVE gap per element between the reference's fp32 and float64 runs.
--check regenerates in memory and compares with the committed file instead of writing it.  The file holds arrays only.
Takes a few minutes: the reference solves M N unit systems in a double Python loop each.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.triag_ref import DIAG_CASES, SOLVE_CASES, make_case  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'triag.npz')


def reference_module(reference_root):
    sys.path.insert(0, reference_root)
    import utils.triag_solve as T

    def with_d(fn):
        def call(A, B, C, *rest):
            if len(rest) == 1:  # (A, B, C, X): the signature before D was added
                rest = (torch.zeros(A.shape[0], A.shape[1], A.shape[2] - 1, A.shape[3] - 1, dtype=A.dtype), rest[0])
            return fn(A, B, C, *rest)
        return call
    T.triag_solve_cuda = types.SimpleNamespace(forward_substitution=with_d(T.forward_substitution),
                                               backward_substitution=with_d(T.backward_substitution))
    return T


def run_solve(fn, case, dtype):
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(k != 'gY') for k, v in case.items()}
    Y = fn.apply(t['A'], t['B'], t['C'], t['D'], t['X'])
    Y.backward(t['gY'])
    out = {'Y': Y.detach()}
    out.update({'g' + k: t[k].grad for k in 'XABCD'})
    return {k: v.numpy() for k, v in out.items()}


def generate(reference_root):
    T = reference_module(reference_root)
    out = {}
    for tag, shape in SOLVE_CASES.items():
        case = make_case(*shape)
        for k, v in case.items():
            out['%s_%s' % (k, tag)] = v
        for d, fn in (('lo', T.ForwardSubst), ('up', T.BackwardSubst)):
            r64, r32 = run_solve(fn, case, torch.float64), run_solve(fn, case, torch.float32)
            for k, v in r64.items():
                out['%s_%s_%s' % (k, d, tag)] = v
                scale = np.abs(v).max() if v.size else 1.0
                gap = np.abs(r32[k].astype(np.float64) - v).max() if v.size else 0.0
                out['noise_%s_%s_%s' % (k, d, tag)] = np.float64(gap / scale)
    for tag, shape in DIAG_CASES.items():
        case = make_case(*shape)
        abc = [torch.from_numpy(case[k]) for k in 'ABC']
        H64 = T.marginal_variances(*[t.double() for t in abc]).numpy()
        H32 = T.marginal_variances(*abc).numpy()
        for k in 'ABC':
            out['%s_diag_%s' % (k, tag)] = case[k]
        out['H_diag_' + tag] = H64
        out['noise_H_diag_' + tag] = np.float64((np.abs(H32.astype(np.float64) - H64) / H64).max())
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
