#!/usr/bin/env python3
"""tests/golden/flow_eval.npz: seeded inputs (tests/flow_eval_ref.py make_case) and what the REFERENCE's own evaluate_flow
(utils/flow_utils.py:121-183, imported live) returns for them -- dense ground truth, sparse ground truth, sparse ground
truth with moving masks.

    python tools/make_flow_eval_golden.py --reference /path/to/reference [--check]

utils/flow_utils.py imports cv2 at its top and the build machines have none, so a stub module `cv2` is put into
sys.modules first.  Its only function, resize(), is THIS tool's half-pixel bilinear (F.interpolate(mode='bilinear',
align_corners=False) on the [H,W,2] array), the map cv2.INTER_LINEAR documents.  So the fixture pins everything but the
resize to the reference's running code -- masks, both F1 thresholds, the divisions, the batch averages -- and the resize by
formula only.  --check regenerates in memory and compares with the committed file instead of
writing it.  The file holds arrays only.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.flow_eval_ref import make_case  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'flow_eval.npz')
CASES = {'a': (3, 20, 33, 61, 130), 'b': (2, 24, 40, 36, 60)}  # B, h, w, H, W


def cv2_stub():
    m = types.ModuleType('cv2')
    m.INTER_LINEAR = 1

    def resize(src, dsize, interpolation=None):
        W, H = dsize
        t = torch.from_numpy(np.ascontiguousarray(src)).permute(2, 0, 1)[None]
        return F.interpolate(t, (H, W), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).contiguous().numpy()
    m.resize = resize
    return m


def generate(reference_root):
    sys.modules['cv2'] = cv2_stub()
    sys.path.insert(0, reference_root)
    from utils.flow_utils import evaluate_flow
    out = {}
    for tag, shape in CASES.items():
        pred, gt, move = make_case(*shape)
        hwc = lambda t: list(t.permute(0, 2, 3, 1).contiguous().numpy())  # noqa: E731
        out['shape_' + tag] = np.array(shape, np.int32)
        out['pred_' + tag] = pred.numpy()
        out['flow_' + tag] = gt[:, :2].numpy()
        for name, t in (('valid', gt[:, 2:3]), ('noc', gt[:, 3:4]), ('move', move)):
            out['%s_%s' % (name, tag)] = t.numpy().astype(np.uint8)
        out['ref_dense_' + tag] = np.array(evaluate_flow(hwc(gt[:, :2]), hwc(pred)), np.float64)
        out['ref_sparse_' + tag] = np.array(evaluate_flow(hwc(gt), hwc(pred)), np.float64)
        out['ref_move_' + tag] = np.array(evaluate_flow(hwc(gt), hwc(pred), list(move[:, 0].numpy())), np.float64)
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
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v), k
        print('%s reproduced: %d arrays equal' % (os.path.relpath(OUT, ROOT), len(out)))
        return
    np.savez_compressed(OUT, **out)
    print('%s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))
    for k in sorted(out):
        if k.startswith('ref_'):
            print(' ', k, out[k])


if __name__ == '__main__':
    main()
