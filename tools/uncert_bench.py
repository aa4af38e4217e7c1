#!/usr/bin/env python3
"""The measurement cases of DESIGN.md section 19 for the uncertainty-metric kernels: arflow_uncert_prep and
arflow_sparsify_sums at B = 8, 384x640 -> 436x1024, C = 2 (F = 2 fields, K = 25 thresholds: one refinement step of both
curves of the batch), arflow_calib_hist with 100 edges at B = 8, 376x1240 on a smooth entropy map (float4 path, a handful
of bins per wave) and at B = 8, 375x1242 on i.i.d. entropy (the flattened plane is not a multiple of 4: the scalar path; a
wave meets some 40 bins per element slot, the histogram's worst case), and the whole metrics.evaluate_uncertainty.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o un -- python tools/uncert_bench.py

gives the kernel times.  On its own the tool prints one JSON line per case: the algorithmic bytes, for sparsify_sums the
sigmoid count B H W F K, and the call time from device events (launch plus the fold of the rows, a torch reduction)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arflow_amd import functional as AF, metrics  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, spec (MI355X); 6.29e12 measured with a float4 copy


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main(iters=20, warmup=3):
    assert torch.cuda.is_available(), 'needs a GPU'
    g = torch.Generator().manual_seed(0)
    B, h, w, H, W, K = 8, 384, 640, 436, 1024, 25
    pred = (torch.randn(B, 2, h, w, generator=g) * 5).cuda()
    gt = (torch.randn(B, 2, H, W, generator=g) * 8).cuda()
    ent = (torch.randn(B, 2, h, w, generator=g) * 0.8 - 0.5).cuda()
    _, epe = AF.flow_eval_sums(pred, gt, want_map=True)
    emap, stats = AF.uncert_prep(ent, epe, gt)
    step = torch.arange(K, device='cuda', dtype=torch.float64) / (K - 1)
    lo, hi = stats[:, [0, 2]] - 0.1, stats[:, [1, 3]] + 0.1
    thr = (hi[..., None] + (lo - hi)[..., None] * step).contiguous()
    out = [('uncert_prep', 4 * B * (2 * h * w + 2 * H * W), None, lambda: AF.uncert_prep(ent, epe, gt)),
           ('sparsify_sums', 4 * B * 2 * H * W, B * H * W * 2 * K, lambda: AF.sparsify_sums(epe, emap, epe, gt, thr, 100.0)),
           ('evaluate_uncertainty', None, 11 * B * H * W * 2 * K, lambda: metrics.evaluate_uncertainty(gt, pred, ent))]
    cc = metrics.CalibrationCurve()
    edges = cc.edges('cuda')
    # the histogram twice: a smooth entropy map on the float4 path (a wave meets a handful of bins: the case the per-wave
    # distinct-bin walk is designed for) and i.i.d. entropy on the scalar path (its worst case: some 40 bins per wave)
    for name, (Hc, Wc), smooth in (('calib_hist_smooth', (376, 1240), True), ('calib_hist_iid', (375, 1242), False)):
        p2 = (torch.randn(B, 2, Hc, Wc, generator=g) * 5).cuda()
        g2 = (torch.randn(B, 2, Hc, Wc, generator=g) * 5).cuda()
        if smooth:
            yy, xx = torch.meshgrid(torch.arange(Hc) / Hc, torch.arange(Wc) / Wc, indexing='ij')
            e2 = -0.3 + 1.3 * torch.sin(6.283 * (1.3 * xx + 0.8 * yy))[None, None] + 0.02 * torch.randn(B, 2, Hc, Wc, generator=g)
        else:
            e2 = torch.randn(B, 2, Hc, Wc, generator=g) * 0.8 - 0.5
        e2 = e2.cuda()
        out.append((name, 4 * B * 6 * Hc * Wc, None, lambda p2=p2, g2=g2, e2=e2: AF.calib_hist_sums(p2, g2, e2, edges)))
    for name, nbytes, sig, fn in out:
        us = timed(fn, iters, warmup)
        line = {'case': name, 'call_us': us, 'iters': iters}
        if nbytes:
            line.update(algorithmic_bytes=nbytes, floor_us_at_spec_peak=nbytes / HBM_PEAK * 1e6)
        if sig:
            line.update(sigmoids=sig, sigmoids_per_s_of_call=sig / (us * 1e-6))
        print(json.dumps(line))


if __name__ == '__main__':
    main()
