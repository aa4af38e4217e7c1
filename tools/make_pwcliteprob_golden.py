#!/usr/bin/env python3
"""tests/golden/elbo_pyramid.npz (loss cases) and tests/golden/elbo_pyramid_models.npz (model cases; a file of its own because no
committed file may exceed 1 MiB): seeded inputs (tests/gauss_pyr_ref.py) and what the REFERENCE's own ElboLoss and PWCLiteProb
(losses/elbo_loss.py, models/pwclite_prob.py, imported live) compute for them on the CPU.

    python tools/make_pwcliteprob_golden.py --reference /path/to/reference [--check]

The loss is built with ElboLoss.__new__ + nn.Module.__init__ + cfg + a CPU Normal(0, 1) (its constructor moves the
distribution to a GPU); for the duration of a call Normal.sample hands out the recorded noise in the order the loss asks for it
(per computed scale: forward, then backward).  Every case runs in float64 and in fp32.

Loss cases (gauss_pyr_ref.LOSS_CASES; B = 2, 32 x 64 images, nets at 32 x 64 ... 2 x 4).  The inputs are shared by the cases:
  seed                      the seed the inputs were made with (see below)
  img, net_<i>, eps_<i>     fp32 inputs: images [2,6,32,64], nets [2,8,h,w], noise [2,4,h,w] (0:2 forward, 2:4 backward)
  <output>_<case>           float64 run: total, warp, smooth, entropy, absmean; mask1_, mask2_<case>: the scale-0 masks;
                            gnet<i>_<case>: the gradient of total w.r.t. net i
  noise_<output>_<case>     max |fp32 run - float64 run| / max |float64 run| of the reference itself
A seed is REFUSED when, in any case, the fp32 and float64 runs disagree on a scale-0 mask pixel, or a pixel of the thresholded
quantity (the clamped correspondence map against 0.2 with occ_from_back, |f12 + f21w|^2 - (0.01 mag + 0.5) otherwise) lies
within 1e-4 of its threshold; the tool then moves to the next seed and prints which one it kept.
Model cases (gauss_pyr_ref.MODEL_CASES; 128 x 192, fill_deterministic weights, eval mode, both directions):
  insum_<case>, keys_<case>, params_<case>, out_<case>_<fw|bw>_<level>  (x4 outputs pooled back by 4)
The tool asserts that clamp(max=10) binds in `clamp` and does not in `U0`.
--check regenerates in memory and compares with the committed files instead of writing them.  The files hold arrays only.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from arflow_amd.config import AttrDict  # noqa: E402
from tests import gauss_pyr_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'elbo_pyramid.npz')
OUT_MODELS = os.path.join(ROOT, 'tests', 'golden', 'elbo_pyramid_models.npz')
FIRST_SEED = 5100


def build_loss(module, cfg):
    loss = module.ElboLoss.__new__(module.ElboLoss)
    torch.nn.Module.__init__(loss)
    loss.cfg = cfg
    loss.Normal = torch.distributions.Normal(0, 1)
    return loss


def run_loss(module, warp_utils, tag, inp, dtype):
    """-> outputs (numpy, `dtype`), and the smallest distance of the thresholded quantity from its threshold."""
    cfg = R.loss_cfg(tag)
    nets = [inp['net_%d' % i].to(dtype).clone().requires_grad_(True) for i in range(len(R.LOSS_SIZES))]
    queue = []
    for i in R.computed_scales(cfg):
        e = inp['eps_%d' % i].to(dtype)
        queue += [e[:, 0:2], e[:, 2:4]]
    first = [queue[0], queue[1]]
    loss = build_loss(module, cfg)
    Normal = torch.distributions.Normal
    saved = Normal.sample

    def sample(self, size=torch.Size()):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(size), (tuple(t.shape), tuple(size))
        return t
    Normal.sample = sample
    try:
        res = loss(nets, inp['img'].to(dtype))
    finally:
        Normal.sample = saved
    assert not queue
    grads = torch.autograd.grad(res[0], nets, allow_unused=True)
    out = dict(zip(R.LOSS_OUTPUTS, res))
    out.update(mask1=loss.pyramid_occu_mask1[0], mask2=loss.pyramid_occu_mask2[0])
    for i, g in enumerate(grads):
        out['gnet%d' % i] = torch.zeros_like(nets[i]) if g is None else g
    # the thresholded quantity of the scale-0 masks, from the same samples
    with torch.no_grad():
        n0 = nets[0]
        zf = n0[:, 0:2] + torch.exp(n0[:, 2:4] / 2.0) * first[0]
        zb = n0[:, 4:6] + torch.exp(n0[:, 6:8] / 2.0) * first[1]
        if cfg.occ_from_back:
            B, _, H, W = zf.shape
            grid = warp_utils.mesh_grid(B, H, W).type_as(zf)
            margin = min(float((warp_utils.get_corresponding_map(grid + f).clamp(min=0., max=1.) - 0.2).abs().min()) for f in (zb, zf))
        else:
            def dist(f12, f21):
                w = warp_utils.flow_warp(f21, f12, pad='zeros')
                mag = (f12 * f12).sum(1, keepdim=True) + (w * w).sum(1, keepdim=True)
                return float((((f12 + w) ** 2).sum(1, keepdim=True) - (0.01 * mag + 0.5)).abs().min())
            margin = min(dist(zf, zb), dist(zb, zf))
    return {k: torch.as_tensor(v).detach().to(dtype).numpy() for k, v in out.items()}, margin


def loss_cases(module, warp_utils):
    seed = FIRST_SEED
    while True:
        inp = R.make_loss_inputs(seed)
        out, why = {}, None
        for tag in R.LOSS_CASES:
            r64, m64 = run_loss(module, warp_utils, tag, inp, torch.float64)
            r32, m32 = run_loss(module, warp_utils, tag, inp, torch.float32)
            if not (np.array_equal(r64['mask1'], r32['mask1']) and np.array_equal(r64['mask2'], r32['mask2'])):
                why = '%s: the fp32 and float64 runs disagree on a scale-0 mask pixel' % tag
            elif min(m64, m32) <= R.MASK_MARGIN:
                why = '%s: a pixel lies %.2e from its threshold' % (tag, min(m64, m32))
            if why:
                break
            for k, v in r64.items():
                out['%s_%s' % (k, tag)] = v
                if k in R.LOSS_OUTPUTS or k.startswith('gnet'):
                    scale = np.abs(v).max()
                    gap = np.abs(r32[k].astype(np.float64) - v).max()
                    out['noise_%s_%s' % (k, tag)] = np.float64(gap / scale if scale > 0 else gap)
        if why is None:
            print('loss cases: kept seed %d' % seed)
            out.update({k: v.numpy() for k, v in inp.items()})
            out['seed'] = np.int64(seed)
            return out
        print('loss cases: seed %d refused (%s)' % (seed, why))
        seed += 1


def model_cases(P):
    out = {}
    torch.set_num_threads(8)
    peak = {}
    for tag in R.MODEL_CASES:
        x, insum = R.make_model_input(tag)
        model = R.prepare(P.PWCLiteProb(R.model_cfg(tag)), tag)
        out['keys_' + tag] = np.array(list(model.state_dict().keys()))
        out['params_' + tag] = np.int64(sum(p.numel() for p in model.parameters()))
        out['insum_' + tag] = np.float64(insum)
        with torch.no_grad():
            res = model(x, with_bk=True)
        assert len(res['flows_fw']) == 5 and len(res['flows_bw']) == 5
        peak[tag] = max(float(f[:, 2:4].max()) for k in res for f in res[k])
        out.update(R.collect(res, tag))
    assert peak['clamp'] == 10.0, 'clamp(max=10) does not bind in the clamp case (peak %.3f)' % peak['clamp']
    assert peak['U0'] < 10.0, 'clamp(max=10) binds in U0 (peak %.3f)' % peak['U0']
    print('model cases: largest log-variance U0 %.3f, U1 %.3f, clamp %.3f' % (peak['U0'], peak['U1'], peak['clamp']))
    return out


def generate(reference_root):
    if 'easydict' not in sys.modules:
        mod = types.ModuleType('easydict')
        mod.EasyDict = AttrDict
        sys.modules['easydict'] = mod
    sys.path.insert(0, reference_root)
    import losses.elbo_loss as L
    import models.pwclite_prob as P
    import utils.warp_utils as WU
    return {OUT: loss_cases(L, WU), OUT_MODELS: model_cases(P)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ARFLOW_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--check', action='store_true', help='compare with the committed files, write nothing')
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('give --reference (or set ARFLOW_REFERENCE)')
    for path, out in generate(os.path.abspath(args.reference)).items():
        if args.check:
            old = np.load(path, allow_pickle=False)
            assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
            for k, v in out.items():
                assert old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v), k
            print('%s reproduced: %d arrays equal' % (os.path.relpath(path, ROOT), len(out)))
            continue
        np.savez_compressed(path, **out)
        print('%s: %d bytes' % (os.path.relpath(path, ROOT), os.path.getsize(path)))
        for k in sorted(out):
            if k.startswith('noise_') and not k.startswith('noise_gnet'):
                print('  %-32s %.3e' % (k, out[k]))


if __name__ == '__main__':
    main()
