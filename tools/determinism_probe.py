"""Is one training step bitwise reproducible in deterministic mode, and if not, where does it first differ?

Runs the forward + loss + backward of one TrainStep workload TWICE from the same seed (same weights, same level-dropout
draws, same images) with arflow_amd's deterministic mode on and torch.backends.cudnn.deterministic = True / benchmark =
False, and compares, in backward order: the loss, every flow the model returned (finest first: the last one produced), the
gradient of every flow, then every parameter gradient from the last layer of the model to the first.  The first tensor
that differs is where the remaining non-determinism enters the backward pass; everything after it inherits the difference.

    python tools/determinism_probe.py [--workload NAME ...] [--size H W] [--batch N] [--default-mode]

--default-mode runs the same comparison with the mode off (how far the atomics move the gradients).  One JSON line per
workload on stdout; exit status 0 whatever the outcome (it is a probe, not a test).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def one_pass(workload, size, batch, device):
    from arflow_amd.train_step import TrainStep, synthetic_pairs
    step = TrainStep(workload, device, seed=1234)
    torch.manual_seed(1000)  # the level-dropout draws
    img = synthetic_pairs(batch, size[0], size[1], frames=step.model_cfg.get('n_frames', 2), device=device, seed=100)
    res = step.model(img, with_bk=True)
    if step.loss_cfg.type == 'mv':
        flows = list(res['flows_fw']) + list(res['flows_bw'])
        out = step.loss(res['flows_fw'], res['flows_bw'], img)
    else:
        flows = [torch.cat([fw, bw], 1) for fw, bw in zip(res['flows_fw'], res['flows_bw'])]
        out = step.loss(flows, img)
    names = [n for n, _ in step.model.named_parameters()]
    params = [p for _, p in step.model.named_parameters()]
    grads = torch.autograd.grad(out[0], flows + params, allow_unused=True)
    gflows, gparams = grads[:len(flows)], grads[len(flows):]
    record = [('loss', out[0].detach())]
    record += [('flow[%d] %s' % (i, tuple(f.shape)), f.detach()) for i, f in enumerate(flows)]
    record += [('d loss / d flow[%d]' % i, g) for i, g in enumerate(gflows) if g is not None]
    record += [('d loss / d %s' % n, g) for n, g in reversed(list(zip(names, gparams))) if g is not None]
    torch.cuda.synchronize()
    return [(n, t.clone()) for n, t in record]


def compare(a, b):
    first, n_diff, worst = None, 0, (0.0, None)
    for (name, x), (_, y) in zip(a, b):
        if torch.equal(x, y):
            continue
        n_diff += 1
        rel = float((x.double() - y.double()).abs().max()) / (float(y.double().abs().max()) + 1e-30)
        if first is None:
            first = {'tensor': name, 'elements_differing': int((x != y).sum()), 'elements': x.numel(), 'max_rel_diff': rel}
        if rel > worst[0]:
            worst = (rel, name)
    return {'bitwise_equal': n_diff == 0, 'tensors': len(a), 'tensors_differing': n_diff, 'first_difference': first,
            'worst_rel_diff': worst[0], 'worst_tensor': worst[1]}


def main():
    from arflow_amd.train_step import WORKLOADS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--workload', nargs='*', default=list(WORKLOADS))
    ap.add_argument('--size', type=int, nargs=2, default=[384, 640])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--default-mode', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('determinism_probe.py needs a GPU')
    from arflow_amd import functional as AF
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    device = torch.device('cuda', 0)
    for workload in args.workload:
        with AF.deterministic(not args.default_mode):
            a = one_pass(workload, args.size, args.batch, device)
            b = one_pass(workload, args.size, args.batch, device)
        line = {'workload': workload, 'size': args.size, 'batch': args.batch, 'deterministic_mode': not args.default_mode}
        line.update(compare(a, b))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
