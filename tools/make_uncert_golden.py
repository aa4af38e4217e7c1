#!/usr/bin/env python3
"""tests/golden/uncert.npz: seeded inputs (tests/uncert_ref.py make_case) and what the REFERENCE's own evaluate_uncertainty,
sp_plot and CalibrationCurve (utils/flow_utils.py:186-320, imported live) return for them.

    python tools/make_uncert_golden.py --reference /path/to/reference [--check] [--time]

As tools/make_flow_eval_golden.py: utils/flow_utils.py imports cv2 at its top and the build machines have none, so a stub
module `cv2` whose resize() is THIS tool's half-pixel bilinear is put into sys.modules first -- the fixture pins everything
but the resize to the reference's running code, and the resize by formula only.  scipy (expit) is the
real one.  Two things the reference keeps to itself are recorded while it runs, without touching its code: the fields it
hands to sp_plot (a wrapper around flow_utils.sp_plot) and the value of every convergence check max|frac - grid_frac| (a
proxy for the module's `np` whose max() notes the calls made from sp_plot's `frac - grid_frac` lines).  The same proxy keeps sp_plot in the float64
arithmetic it was written under: the reference predates NumPy 2, where `np.max(entropy) + eps` (np.float32 + float) was a
float64 and so was the threshold grid; under NumPy >= 2 the sum stays float32, np.linspace of two float32 scalars is a
float32 grid and the first evaluation of every curve silently runs in float32.  The proxy's max() / min() of a 2-D field
return the float32 extreme as an np.float64, which restores the former on either NumPy.

Per case: the inputs; evaluate_uncertainty's pair and curves; the recorded fields and checks; for a same-size case the
four lists of CalibrationCurve; and `sens`, the noise floor: the largest change of each output over 8 seeded draws of
absolute noise 8 * 2^-24 * A on the flows (A = max(|gt|, |scaled pred|)) and 8 * 2^-24 * max|entropy| on the entropy -- the
size of the rounding an fp32 implementation of the resize and the error map carries.  (For the calibration lists only the
flows are perturbed: noise on the entropy moves elements between bins, which the tests bound by the edge band instead.)

Two conditions on the INPUTS are asserted on the reference alone: every recorded check is at least 1e-3 away from eps, so
no rounding flips a convergence decision; and at most 0.5 % of the calibration elements have sigma within 4 float32 ulps of
a bin edge.  --check regenerates in memory and compares with the committed file; --time also prints the reference's host
time for B = 8, 384x640 -> 436x1024 (a baseline for DESIGN.md section 19, not stored).  The file holds arrays only.
"""
import argparse
import linecache
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import uncert_ref as U  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'uncert.npz')
# tag: (B, h, w, H, W, C)
CASES = {'a': (2, 20, 33, 61, 130, 4), 'b': (2, 36, 60, 36, 60, 4), 'c': (1, 24, 40, 48, 80, 2)}
N = 25
DRAWS = 8
MAXCHECKS = U.REFINEMENTS + 2


def cv2_stub():
    m = types.ModuleType('cv2')
    m.INTER_LINEAR = 1

    def resize(src, dsize, interpolation=None):
        W, H = dsize
        t = torch.from_numpy(np.ascontiguousarray(src)).permute(2, 0, 1)[None]
        return F.interpolate(t, (H, W), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).contiguous().numpy()
    m.resize = resize
    return m


class Recorder:
    """What the reference computes on the way, noted while it runs."""

    def __init__(self, fu):
        self.fu, self.fields, self.checks = fu, [], []
        inner, rec = fu.sp_plot, self

        class NP:
            def __getattr__(self, name):
                return getattr(np, name)

            @staticmethod
            def max(a, *args, **kw):
                r = np.max(a, *args, **kw)
                caller = sys._getframe(1)
                line = linecache.getline(caller.f_code.co_filename, caller.f_lineno)
                if caller.f_code.co_name == 'sp_plot' and 'frac - grid_frac' in line:  # the convergence checks only
                    rec.checks[-1].append(float(r))
                return np.float64(r) if isinstance(a, np.ndarray) and a.ndim == 2 else r

            @staticmethod
            def min(a, *args, **kw):
                r = np.min(a, *args, **kw)
                return np.float64(r) if isinstance(a, np.ndarray) and a.ndim == 2 else r

        def sp_plot(error, entropy, gt_mask, *args, **kw):
            rec.fields.append((np.array(error), np.array(entropy), np.array(gt_mask)))
            rec.checks.append([])
            return inner(error, entropy, gt_mask, *args, **kw)
        fu.np, fu.sp_plot = NP(), sp_plot

    def take(self):
        f, c = self.fields, self.checks
        self.fields, self.checks = [], []
        return f, c


def hwc(t):
    return list(t.permute(0, 2, 3, 1).contiguous().numpy())


def run_reference(fu, rec, pred, gt, ent, calib):
    """-> dict of float64 arrays (+ the recorded float32 fields)."""
    B = gt.shape[0]
    pair, splots, oracle = fu.evaluate_uncertainty(hwc(gt), hwc(pred), hwc(ent), sp_samples=N)
    fields, checks = rec.take()
    assert len(fields) == 2 * B
    resid = np.full((B, 2, MAXCHECKS), np.nan)
    for i, c in enumerate(checks):
        resid[i // 2, i % 2, :len(c)] = c
    out = {'pair': np.array(pair, np.float64), 'splots': np.array(splots, np.float64),
           'oracle_splots': np.array(oracle, np.float64), 'resid': resid,
           'epe': np.stack([fields[2 * b][0] for b in range(B)]), 'ent_map': np.stack([fields[2 * b][1] for b in range(B)])}
    assert out['epe'].dtype == np.float32 and out['ent_map'].dtype == np.float32
    if calib:
        cc = fu.CalibrationCurve()
        cc(hwc(gt), hwc(pred), hwc(ent))
        import contextlib
        import io
        import warnings
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter('ignore')  # the mean of an empty bin
            vals, means, sigmas, numbers = cc.calibration_curve()
        out.update(cc_vals=np.array(vals, np.float64), cc_means=np.array(means, np.float64),
                   cc_sigmas=np.array(sigmas, np.float64), cc_numbers=np.array(numbers, np.int64))
    return out


def generate(reference_root, verbose=True):
    sys.modules['cv2'] = cv2_stub()
    sys.path.insert(0, reference_root)
    from utils import flow_utils as fu
    rec = Recorder(fu)
    out = {}
    for tag, shape in CASES.items():
        B, h, w, H, W, C = shape
        calib = (h, w) == (H, W)
        pred, gt, ent = U.make_case(*shape)
        base = run_reference(fu, rec, pred, gt, ent, calib)
        # condition 1: no convergence decision within 1e-3 of eps
        gap = np.nanmin(np.abs(base['resid'] - U.EPS))
        assert gap >= 1e-3, (tag, gap)
        steps = [[U.steps_of(base['resid'][b, f]) for f in range(2)] for b in range(B)]
        # condition 2: the edge band of the calibration bins
        band = None
        if calib:
            _, band = U.calib_hist(pred, gt, ent, np.linspace(0, 3.5, 100))
            assert band <= 0.005 * ent.numel(), (tag, band)
        # the noise floor
        scaled = torch.stack([pred[:, 0] / w * W, pred[:, 1] / h * H], 1)
        A = float(max(gt[:, :2].abs().max(), scaled.abs().max()))
        nf, ne = 8 * 2.0 ** -24 * A, 8 * 2.0 ** -24 * float(ent.abs().max())
        sens = {k: np.zeros_like(v, dtype=np.float64) for k, v in base.items() if k in ('pair', 'splots', 'oracle_splots')}
        csens = {k: np.zeros_like(base[k]) for k in ('cc_means', 'cc_sigmas')} if calib else {}
        rng = np.random.default_rng(99)
        unit = torch.tensor([w / W, h / H], dtype=torch.float32).view(1, 2, 1, 1)
        for _ in range(DRAWS):
            noise = lambda t, a: torch.from_numpy(rng.uniform(-a, a, tuple(t.shape)).astype(np.float32))  # noqa: E731
            gt2 = gt.clone()
            gt2[:, :2] += noise(gt[:, :2], nf)
            pred2 = pred + noise(pred, nf) * unit
            got = run_reference(fu, rec, pred2, gt2, ent + noise(ent, ne), False)
            assert np.nanmin(np.abs(got['resid'] - U.EPS)) >= 1e-3
            for k in sens:
                sens[k] = np.maximum(sens[k], np.abs(got[k] - base[k]))
            if calib:
                got = run_reference(fu, rec, pred2, gt2, ent, True)
                assert np.array_equal(got['cc_numbers'], base['cc_numbers'])
                for k in csens:
                    d = np.abs(got[k] - base[k])
                    csens[k] = np.maximum(csens[k], np.where(np.isnan(d), 0.0, d))
        out['shape_' + tag] = np.array(shape, np.int32)
        out['pred_' + tag], out['flow_' + tag], out['ent_' + tag] = pred.numpy(), gt[:, :2].numpy(), ent.numpy()
        if C == 4:
            out['valid_' + tag], out['noc_' + tag] = gt[:, 2].numpy().astype(np.uint8), gt[:, 3].numpy().astype(np.uint8)
        for k, v in base.items():
            out['ref_%s_%s' % (k, tag)] = v
        for k, v in {**sens, **csens}.items():
            out['sens_%s_%s' % (k, tag)] = v
        if verbose:
            print('case %s %s: pair %s  steps %s  closest check to eps %.4f  edge band %s of %d  A %.2f' %
                  (tag, shape, base['pair'], steps, gap, band, ent.numel(), A))
            print('   sens: pair %s  splot rel %.3g  oracle rel %.3g' % (
                sens['pair'], (sens['splots'] / np.abs(base['splots'])).max(),
                (sens['oracle_splots'] / np.abs(base['oracle_splots'])).max())
                + ('  cc means %.3g sigmas %.3g' % (csens['cc_means'].max(), csens['cc_sigmas'].max()) if calib else ''))
    return out, fu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ARFLOW_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--check', action='store_true', help='compare with the committed file, write nothing')
    ap.add_argument('--time', action='store_true', help='also time the reference at B = 8, 384x640 -> 436x1024')
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('give --reference (or set ARFLOW_REFERENCE)')
    out, fu = generate(os.path.abspath(args.reference))
    if args.check:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for k, v in out.items():
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v, equal_nan=v.dtype.kind == 'f'), k
        print('%s reproduced: %d arrays equal' % (os.path.relpath(OUT, ROOT), len(out)))
    else:
        np.savez_compressed(OUT, **out)
        print('%s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))
    if args.time:
        pred, gt, ent = U.make_case(8, 384, 640, 436, 1024, C=2)
        t0 = time.perf_counter()
        pair, _, _ = fu.evaluate_uncertainty(hwc(gt), hwc(pred), hwc(ent), sp_samples=N)
        print('reference evaluate_uncertainty, B = 8, 384x640 -> 436x1024, host: %.2f s (pair %s)' %
              (time.perf_counter() - t0, pair))


if __name__ == '__main__':
    main()
