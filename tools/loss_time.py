"""Time one pyramid loss alone: forward + backward of the loss of a train_step.WORKLOADS entry on fixed flows
(requires_grad leaves of the model's output shapes) at 8 x 384x640, HIP events around every iteration, warm,
median over --iters iterations.  Uses only the losses' public interface, so the same file runs on an older checkout
for an A/B; ARFLOW_PHOTO_WARP=0 selects the composed path where the switch exists.

    python tools/loss_time.py --workload pwclite+unflow_loss --iters 100
prints one JSON line: {"workload", "median_ms", "min_ms", "p90_ms", "iters", "abi_calls"}."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='pwclite+unflow_loss', choices=['pwclite+unflow_loss', 'pwclite3+mv_loss'])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=[384, 640])
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    from arflow_amd import functional as AF
    from arflow_amd.config import AttrDict
    from arflow_amd.losses import get_loss
    from arflow_amd.train_step import WORKLOADS, synthetic_pairs
    cfg = AttrDict(WORKLOADS[a.workload][1])
    B, (H, W) = a.batch, a.size
    gen = torch.Generator().manual_seed(3)
    sizes = ([(H, W)] + [(H // s, W // s) for s in (4, 8, 16, 32, 64)])[:len(cfg.w_scales)]
    loss = get_loss(cfg)

    def flows(ch):
        out = []
        for h, w in sizes:
            coarse = 0.02 * h * torch.randn(B, ch, 3, 5, generator=gen)
            f = torch.nn.functional.interpolate(coarse, (h, w), mode='bilinear', align_corners=True) + \
                0.05 * torch.randn(B, ch, h, w, generator=gen)
            out.append(f.cuda().requires_grad_(True))
        return out
    if cfg.type == 'mv':
        img = synthetic_pairs(B, H, W, frames=3)
        f12, f10 = flows(2), flows(2)
        args, leaves = (f12, f10, img), f12 + f10
    else:
        img = synthetic_pairs(B, H, W, frames=2)
        fl = flows(4)
        args, leaves = (fl, img), fl

    def step():
        for t in leaves:
            t.grad = None
        loss(*args)[0].backward()

    for _ in range(a.warmup):
        step()
    AF.start_kernel_timing()
    step()
    calls = sum(len(v) for v in AF.stop_kernel_timing().values())
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    print(json.dumps({'workload': a.workload, 'median_ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4),
                      'p90_ms': round(ms[int(0.9 * (len(ms) - 1))], 4), 'iters': a.iters, 'abi_calls': calls}))


if __name__ == '__main__':
    main()
