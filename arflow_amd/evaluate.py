#!/usr/bin/env python3
"""Score predicted flows against ground truth with the reference's metrics (utils/flow_utils.py:121-183).

    python -m arflow_amd.evaluate --pred A --gt B [--entropy E [--calibration]]

A and B are two .flo files, or two directories whose .flo files are matched by name.  A prediction of another size is
scaled and resized to its ground truth as the reference does.  Prints one JSON line: the metric names, their means over
the pairs, and the pair count.  Runs on the GPU through arflow_flow_eval.

E is the predicted entropy: an .npy file, or a directory whose .npy files are matched to the .flo names by stem; each
holds an [h,w,2] array of the prediction's size, as the reference's inference.py:104-114 writes it.  The line then gains
AUC, AUC_diff and not_converged (evaluate_uncertainty of utils/flow_utils.py:281-320; evaluate_flo_files_sintel.py), and
with --calibration the four lists of CalibrationCurve.calibration_curve() as cc_vals, cc_means, cc_sigmas, cc_numbers (the
mean of an empty bin is NaN, which json writes as the bare word NaN); the calibration needs predictions of the ground
truth's size.
"""
import argparse
import json
import os

import numpy as np
import torch

from .flow_io import read_flow
from .metrics import CalibrationCurve, FlowMetrics, UncertaintyMetrics


def _pairs(pred, gt):
    if os.path.isdir(pred) != os.path.isdir(gt):
        raise SystemExit('--pred and --gt must be two files or two directories')
    if not os.path.isdir(pred):
        return [(pred, gt)]
    names = sorted(n for n in os.listdir(gt) if n.endswith('.flo'))
    missing = [n for n in names if not os.path.exists(os.path.join(pred, n))]
    if missing or not names:
        raise SystemExit('no prediction for %s' % ', '.join(missing) if missing else 'no .flo files in %s' % gt)
    return [(os.path.join(pred, n), os.path.join(gt, n)) for n in names]


def _entropy_paths(pairs, entropy, from_dirs):
    """The .npy file of every (prediction, ground truth) pair: `entropy` itself for two files, <stem>.npy in it for two
    directories."""
    if os.path.isdir(entropy) != from_dirs:
        raise SystemExit('--entropy must be an .npy file for two .flo files, a directory for two directories')
    if not os.path.isdir(entropy):
        if not os.path.exists(entropy):
            raise SystemExit('no entropy file %s' % entropy)
        return [entropy]
    paths = [os.path.join(entropy, os.path.splitext(os.path.basename(p))[0] + '.npy') for p, _ in pairs]
    missing = [os.path.basename(e) for e in paths if not os.path.exists(e)]
    if missing:
        raise SystemExit('no entropy for %s in %s' % (', '.join(missing), entropy))
    return paths


def _load_entropy(path, like, device):
    a = np.load(path, allow_pickle=False)
    if a.ndim != 3 or a.shape[2] != 2 or a.shape[:2] != tuple(like.shape[2:]):
        raise SystemExit('%s: expected an entropy array [%d,%d,2], got %s' % (path, like.shape[2], like.shape[3], a.shape))
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).permute(2, 0, 1)[None].contiguous().to(device)


def _load(path, device):
    return torch.from_numpy(read_flow(path).copy()).permute(2, 0, 1)[None].contiguous().to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--pred', required=True, help='.flo file or directory of predictions')
    ap.add_argument('--gt', required=True, help='.flo file or directory of ground-truth flows')
    ap.add_argument('--entropy', help='.npy file or directory of predicted entropies [h,w,2]: adds AUC, AUC_diff')
    ap.add_argument('--calibration', action='store_true', help='with --entropy: add the calibration curve')
    args = ap.parse_args(argv)
    if args.calibration and not args.entropy:
        raise SystemExit('--calibration needs --entropy')
    pairs = _pairs(args.pred, args.gt)
    entropies = _entropy_paths(pairs, args.entropy, os.path.isdir(args.pred)) if args.entropy else None
    if not torch.cuda.is_available():
        raise SystemExit('arflow_amd.evaluate needs a GPU: the metric kernel has no CPU fallback')
    device = torch.device('cuda')
    meter = FlowMetrics()
    umeter = UncertaintyMetrics() if entropies else None
    curve = CalibrationCurve() if args.calibration else None
    for i, (p, g) in enumerate(pairs):
        pred, gt = _load(p, device), _load(g, device)
        meter.update(pred, gt)
        if umeter is not None:
            ent = _load_entropy(entropies[i], pred, device)
            umeter.update(pred, gt, ent)
            if curve is not None:
                curve.update(pred, gt, ent)
    out = dict(meter.compute(), pairs=len(pairs))
    if umeter is not None:
        u = umeter.compute()
        out.update(AUC=u['AUC'], AUC_diff=u['AUC_diff'], not_converged=u['not_converged'])
    if curve is not None:
        out.update(zip(('cc_vals', 'cc_means', 'cc_sigmas', 'cc_numbers'), curve.calibration_curve()))
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
