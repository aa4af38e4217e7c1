#!/usr/bin/env python3
"""The two measurement cases of DESIGN.md section 15 for arflow_flow_eval: dense ground truth (B = 8, 384x640 -> 436x1024,
C = 2: the float4 path) and sparse ground truth (256x832 -> 375x1242, C = 4, W % 4 != 0: the scalar path).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fe -- python tools/flow_eval_bench.py

gives the kernel time (flow_eval_kernel<true> is the dense case, <false> the sparse one).  On its own the tool prints one
JSON line per case: the algorithmic bytes 4 B (C H W + 2 h w [+ H W]) and the call time from device events (the launch
plus the fold of the rows, a torch reduction)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arflow_amd import functional as AF  # noqa: E402

CASES = {'dense': (8, 384, 640, 436, 1024, 2), 'sparse': (8, 256, 832, 375, 1242, 4)}
HBM_PEAK = 8.0e12  # bytes/s, spec (MI355X); 6.29e12 measured with a float4 copy


def main(iters=50, warmup=5):
    assert torch.cuda.is_available(), 'needs a GPU'
    g = torch.Generator().manual_seed(0)
    for name, (B, h, w, H, W, C) in CASES.items():
        pred = (torch.randn(B, 2, h, w, generator=g) * 5).cuda()
        gt = torch.randn(B, C, H, W, generator=g) * 8
        if C == 4:
            gt[:, 2:] = (gt[:, 2:] > 0).float()
        gt = gt.cuda()
        for _ in range(warmup):
            AF.flow_eval_sums(pred, gt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            AF.flow_eval_sums(pred, gt)
        e1.record()
        torch.cuda.synchronize()
        nbytes = 4 * B * (C * H * W + 2 * h * w)
        print(json.dumps({'case': name, 'B': B, 'pred': [h, w], 'gt': [C, H, W], 'algorithmic_bytes': nbytes,
                          'floor_us_at_spec_peak': nbytes / HBM_PEAK * 1e6, 'call_us': e0.elapsed_time(e1) * 1e3 / iters,
                          'iters': iters}))


if __name__ == '__main__':
    main()
