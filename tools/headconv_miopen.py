#!/usr/bin/env python3
"""The two-channel flow heads of the flagship run alone through F.conv2d (MIOpen): HIP-event time per pass and shape,
the figure the native head convolution (csrc/headconv.hip) is set against.  Under `rocprofv3 --kernel-trace --stats`
the same run names MIOpen's kernels for these problems.

    python tools/headconv_miopen.py [--iters 20] [--prob]

--prob: the heads of PWCProbFlow at its training shape instead (2B = 8): 32 -> 4 channels at levels
4..2, 32 -> 34 at level 1 and for the last refinement convolution.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (points MIOpen at the shipped find database, as the benchmark does)
import torch  # noqa: E402

HEAD_SHAPES = [(16, 595, 96, 160), (16, 595, 48, 80), (16, 595, 24, 40), (16, 563, 12, 20), (16, 32, 96, 160)]
# (B, C, H, W, K): level heads 4..1, then the last refinement convolution
PROB_SHAPES = [(8, 32, 12, 20, 4), (8, 32, 24, 40, 4), (8, 32, 48, 80, 4), (8, 32, 96, 160, 34), (8, 32, 96, 160, 34)]


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--prob', action='store_true', help='the 4- and 34-channel heads of PWCProbFlow')
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device='cuda').manual_seed(0)
    cb = torch.ops.aten.convolution_backward
    total = 0.0
    for B, C, H, W, K in (PROB_SHAPES if args.prob else [s + (2,) for s in HEAD_SHAPES]):
        x = torch.randn(B, C, H, W, device=dev, generator=g)
        w = 0.05 * torch.randn(K, C, 3, 3, device=dev, generator=g)
        b = torch.randn(K, device=dev, generator=g)
        dy = torch.randn(B, K, H, W, device=dev, generator=g)
        conv_args = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)
        t = {
            'fwd': timeit(lambda: torch.nn.functional.conv2d(x, w, b, 1, 1), args.iters),
            'dgrad': timeit(lambda: cb(dy, x, w, [K], *conv_args, [True, False, False]), args.iters),
            'wgrad+dbias': timeit(lambda: cb(dy, x, w, [K], *conv_args, [False, True, True]), args.iters),
            'bwd_all': timeit(lambda: cb(dy, x, w, [K], *conv_args, [True, True, True]), args.iters),
        }
        total += t['fwd'] + t['bwd_all']
        print(json.dumps({'shape': [B, C, H, W], 'out_channels': K, 'miopen_us': {k: round(v, 1) for k, v in t.items()},
                          'x_MB': round(4e-6 * B * C * H * W, 1)}), flush=True)
        del x, dy
    print(json.dumps({'fwd_plus_bwd_all_us_over_the_five_heads': round(total, 1)}))


if __name__ == '__main__':
    main()
