#!/usr/bin/env python3
"""tests/golden/render.npz: seeded flows (tests/render_ref.py) and what the REFERENCE's own code makes of them --
np_flow2rgb, torch_flow2rgb, the uint8 cast of trainer/uflow_elbo_trainer.py:244-245 and flow_to_image (max_flow = 256 and
None) of utils/flow_utils.py, imported live, and the restore of inference.py:98-107.

    python tools/make_render_golden.py --reference /path/to/reference [--check]

utils/flow_utils.py imports cv2 at its top and the build machines have none, so a stub module `cv2` is put into sys.modules
first.  Its only function, resize(), is THIS tool's half-pixel bilinear (tests/render_ref.py blend64, evaluated in float64 and
returned in the source's dtype), the map cv2.INTER_LINEAR documents.  inference.py cannot be imported (it needs the datasets
and two packages the machines lack) and its restore is the body of a loop, so the tool reads the reference's file, takes the
statements between its comments '# Resample flow - back to original shape' and '# Store the result', and executes THEM
with the stub as cv2: the arithmetic around the resize is the reference's running code, the resize is pinned by formula only
(parity with cv2's own INTER_LINEAR stays unpinned).  --check regenerates in memory and compares with
the committed file instead of writing it.  The file holds arrays only.
"""
import argparse
import math
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import render_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'render.npz')
RESTORE_CASES = {'up': (2, 12, 20, 31, 53), 'down': (2, 12, 20, 5, 7)}  # B, h, w, H, W
RENDER_CASES = {'s': (2, 5, 7), 'm': (1, 33, 67)}  # B, H, W
MAX_VALUE = 7.5


def cv2_stub():
    m = types.ModuleType('cv2')
    m.INTER_LINEAR = 1

    def resize(src, dsize, interpolation=None):
        W, H = dsize
        out, _ = R.blend64(np.moveaxis(np.asarray(src), -1, 0), (H, W))
        return np.ascontiguousarray(np.moveaxis(out, 0, -1)).astype(src.dtype)
    m.resize = resize
    return m


def restore_statements(reference_root):
    lines = open(os.path.join(reference_root, 'inference.py')).read().split('\n')
    a = next(i for i, s in enumerate(lines) if '# Resample flow - back to original shape' in s)
    b = next(i for i, s in enumerate(lines) if '# Store the result' in s)
    return compile(textwrap.dedent('\n'.join(lines[a:b])), 'inference.py:%d-%d' % (a + 1, b), 'exec')


def generate(reference_root):
    stub = cv2_stub()
    sys.modules['cv2'] = stub
    sys.path.insert(0, reference_root)
    from utils.flow_utils import flow_to_image, np_flow2rgb, torch_flow2rgb
    code = restore_statements(reference_root)
    out = {}
    for tag, (B, h, w, H, W) in RESTORE_CASES.items():
        flow, ent = R.make_flow(R.SEED, B, h, w), R.make_entropy(R.SEED, B, h, w)
        fl, en = [], []
        for b in range(B):  # inference.py:52,88: NHWC numpy views of the network's output
            ns = {'cv2': stub, 'math': math, 'H': H, 'W': W, 'pred_flow': flow[b].transpose(1, 2, 0).copy(),
                  'pred_entropy': ent[b].transpose(1, 2, 0).copy()}
            exec(code, ns)
            fl.append(ns['pred_flow'])
            en.append(ns['pred_entropy'])
        out['shape_' + tag] = np.array((B, h, w, H, W), np.int32)
        out['flow_' + tag], out['ent_' + tag] = flow, ent
        out['ref_flow_' + tag], out['ref_ent_' + tag] = np.stack(fl).astype(np.float32), np.stack(en).astype(np.float32)
    for tag, (B, H, W) in RENDER_CASES.items():
        flow = R.make_flow(R.SEED + 1, B, H, W)
        hwc = flow.transpose(0, 2, 3, 1)
        out['rflow_' + tag] = flow
        out['rgb_val_' + tag] = np.stack([np_flow2rgb(f.copy(), MAX_VALUE) for f in flow])
        image = torch_flow2rgb(torch.from_numpy(flow.copy()))
        out['t2rgb_' + tag] = image.numpy()  # np_flow2rgb(flow, None) per sample, NCHW
        out['t2rgb_u8_' + tag] = (image.numpy().transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)  # uflow_elbo_trainer.py:244-245
        out['wheel_256_' + tag] = np.stack([flow_to_image(f.copy()) for f in hwc])
        out['wheel_none_' + tag] = np.stack([flow_to_image(f.copy(), max_flow=None) for f in hwc])
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
        print(' ', k, out[k].dtype, out[k].shape)


if __name__ == '__main__':
    main()
