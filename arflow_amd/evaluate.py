#!/usr/bin/env python3
"""Score predicted flows against ground truth with the reference's metrics (utils/flow_utils.py:121-183).

    python -m arflow_amd.evaluate --pred A --gt B

A and B are two .flo files, or two directories whose .flo files are matched by name.  A prediction of another size is
scaled and resized to its ground truth as the reference does.  Prints one JSON line: the metric names, their means over
the pairs, and the pair count.  Runs on the GPU through arflow_flow_eval.
"""
import argparse
import json
import os

import torch

from .flow_io import read_flow
from .metrics import FlowMetrics


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


def _load(path, device):
    return torch.from_numpy(read_flow(path).copy()).permute(2, 0, 1)[None].contiguous().to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--pred', required=True, help='.flo file or directory of predictions')
    ap.add_argument('--gt', required=True, help='.flo file or directory of ground-truth flows')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('arflow_amd.evaluate needs a GPU: the metric kernel has no CPU fallback')
    device = torch.device('cuda')
    meter = FlowMetrics()
    pairs = _pairs(args.pred, args.gt)
    for p, g in pairs:
        meter.update(_load(p, device), _load(g, device))
    out = dict(meter.compute(), pairs=len(pairs))
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
