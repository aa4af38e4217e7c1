#!/usr/bin/env python3
"""tests/golden/prob_models.npz: what the REFERENCE's own PWCProbFlow (models/uflow_prob_model.py, imported live) computes
on the CPU for the cases of tests/prob_ref.py -- deterministic weights (oracle.fixture_common.fill_deterministic), one seeded
image pair of 192 x 256, batch 1.

    python tools/make_prob_golden.py --reference /path/to/reference [--check]

The reference imports `easydict`; this tool registers an in-memory module of that name whose EasyDict is
arflow_amd.config.AttrDict before importing it, so nothing has to be installed.

  insum                         float64 sum of the input pair, against a drift of the recipe
  keys_<case>, params_<case>    the state_dict's key order and the parameter count
  out_<case>_<fw|bw>_<level>    the stored channels (tests/prob_ref.py stored_channels) of that output; levels 0 and 1
                                average-pooled to quarter resolution, as models.npz does
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
from tests import prob_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'prob_models.npz')


def generate(reference_root):
    if 'easydict' not in sys.modules:
        mod = types.ModuleType('easydict')
        mod.EasyDict = AttrDict
        sys.modules['easydict'] = mod
    sys.path.insert(0, reference_root)
    import models.uflow_prob_model as P
    img1, img2, insum = R.make_input()
    out = {'insum': np.float64(insum)}
    torch.set_num_threads(8)
    for tag in R.CASES:
        model = R.prepare(P.PWCProbFlow(R.model_cfg(tag)), tag)
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
        if k.startswith('out_'):
            v = out[k]
            print('  %-16s %-18s min %+.4f max %+.4f' % (k, v.shape, v.min(), v.max()))


if __name__ == '__main__':
    main()
