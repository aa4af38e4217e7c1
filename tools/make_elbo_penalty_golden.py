#!/usr/bin/env python3
"""tests/golden/elbo_penalty.npz: seeded inputs (tests/elbo_penalty_ref.py) and what the REFERENCE's own UFlowElboLoss
(losses/uflow_elbo_loss.py, imported live) computes for them with the selectable penalties and occ_type 'mean'.

    python tools/make_elbo_penalty_golden.py --reference /path/to/reference [--check]

As tools/make_elbo_golden.py, the loss's `Normal` is replaced by one that hands out the recorded noise.  The reference's
get_penalty knows identity, charbonnier and abs_robust_loss; for the mixture cases this tool substitutes, in its own process,
the module-level `get_penalty` of the imported loss module by one that adds two callables built on the reference's OWN log_gmm
(losses/uflow_elbo_loss.py:99-105): h -> -log_gmm(h, pi, beta) for the data term and x_sq -> -log_gmm(sqrt(x_sq), pi, beta)
for the smoothness term, with the mixtures of the case's config.  Every case runs in float64 and in fp32; torch's default
dtype is set to the run's dtype, so that the float64 run forms the mixture weights in float64 too (log_gmm builds them with
torch.tensor(pi), which takes the default dtype).

Per case <tag> (tests/elbo_penalty_ref.py CASES; B = 2, 32 x 64 images, an 8 x 16 level 2):
  net12_, net21_, eps12_, eps21_<tag>    the fp32 inputs and the noise; im1_noise / im2_noise, im1_spread / im2_spread: the two
                                         image pairs the cases share
  <output>_<tag>                         the float64 run: total, warp, smooth, entropy, oof, flow12_2, occu_mask12,
                                         valid_mask12, gnet12, gnet21
  noise_<output>_<tag>                   max |fp32 run - float64 run| / max |float64 run| of the reference itself
  hfrac_<tag>  (data cases)              the fractions of unmasked interior pixels with h < 1 and with h > 10 (asserted >= 0.1)
--check regenerates in memory and compares with the committed file instead of writing it.  The file holds arrays only.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import elbo_penalty_ref as P  # noqa: E402
from tests import elbo_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'elbo_penalty.npz')


class Recorded:
    """Stands in for torch.distributions.Normal(0, 1): sample(size) returns the next recorded tensor."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def sample(self, size):
        t = self.tensors.pop(0)
        assert tuple(t.shape) == tuple(size), (tuple(t.shape), tuple(size))
        return t


def reference_cfg(module, tag):
    """The case's config as the reference reads it, and the get_penalty to install: the two mixture callables go by names of
    their own, since the reference asks get_penalty(name) for both terms."""
    cfg = P.case_cfg(tag)
    original = module.get_penalty.__wrapped__ if hasattr(module.get_penalty, '__wrapped__') else module.get_penalty
    census = (list(cfg.penalty_census_pi), list(cfg.penalty_census_beta))
    smooth = (list(cfg.penalty_smooth_pi), list(cfg.penalty_smooth_beta))

    def get_penalty(name, derivative=False):
        if name == 'gmm_census':
            return lambda h: -module.log_gmm(h, *census)
        if name == 'gmm_smooth':
            return lambda x_sq: -module.log_gmm(torch.sqrt(x_sq), *smooth)
        return original(name, derivative)
    get_penalty.__wrapped__ = original
    ref = R.Cfg(dict(cfg))
    if cfg.data_penalty == ['gmm']:
        ref['data_penalty'] = ['gmm_census']
    if cfg.penalty_smooth == 'gmm':
        ref['penalty_smooth'] = 'gmm_smooth'
    return ref, get_penalty


def run_loss(module, tag, case, dtype):
    cfg, module.get_penalty = reference_cfg(module, tag)
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        t = {k: torch.from_numpy(v).to(dtype) for k, v in case.items()}
        net12, net21 = t['net12'].requires_grad_(True), t['net21'].requires_grad_(True)
        loss = module.UFlowElboLoss(cfg)
        loss.Normal = Recorded([t['eps12'], t['eps21']])
        res = loss({'flows_fw': [None, None, net12], 'flows_bw': [None, None, net21]}, t['im1'], t['im2'])
        res[0].backward()
        out = dict(zip(P.OUTPUTS[:8], res))
        out.update(gnet12=net12.grad, gnet21=net21.grad)
        return {k: torch.as_tensor(v, dtype=dtype).detach().numpy() for k, v in out.items()}
    finally:
        torch.set_default_dtype(before)


def spread_of(module, tag, case):
    """fractions of the unmasked interior pixels of the forward direction with h < 1 and with h > 10, from the reference's
    own data_loss_no_penalty on the case's samples"""
    cfg = P.case_cfg(tag)
    t = {k: torch.from_numpy(v).double() for k, v in case.items()}
    res = P.loss(cfg, case)  # the samples (flow12_2) as the loss forms them
    S = cfg.n_samples
    f12 = torch.from_numpy(res['flow12_2'])
    k = cfg.cov_supp if cfg.approx == 'sparse' else 0
    n = (k + 1) ** 2 - 1
    mean21 = t['net21'][:, 0:2]
    z21 = mean21.repeat(S, 1, 1, 1) + R._product_t(torch.cat((torch.exp(t['net21'][:, 2:4]), t['net21'][:, 4:4 + 2 * n]), 1)
                                                    .repeat(S, 1, 1, 1), t['eps21'], k)
    losses, weights, _, _ = module.data_loss_no_penalty(t['im1'].repeat(S, 1, 1, 1), t['im2'].repeat(S, 1, 1, 1), f12, z21,
                                                        cfg.occ_type, cfg.data_loss, t['net12'][:, 0:2].repeat(S, 1, 1, 1),
                                                        mean21.repeat(S, 1, 1, 1))
    h, wgt = losses[0], weights[0]
    keep = wgt > 0.5 * wgt.max()  # unmasked (mask about 1) interior pixels
    return np.array([float((h[keep] < 1).double().mean()), float((h[keep] > 10).double().mean())])


def generate(reference_root):
    sys.path.insert(0, reference_root)
    import losses.uflow_elbo_loss as L
    out = {}
    for tag in P.CASES:
        case = P.make_case(tag)
        kind = P.CASES[tag]['inputs']
        for k in ('im1', 'im2'):
            name = '%s_%s' % (k, kind)
            assert name not in out or np.array_equal(out[name], case[k])
            out[name] = case[k]
        for k in ('net12', 'net21', 'eps12', 'eps21'):
            out['%s_%s' % (k, tag)] = case[k]
        r64, r32 = run_loss(L, tag, case, torch.float64), run_loss(L, tag, case, torch.float32)
        for k, v in r64.items():
            out['%s_%s' % (k, tag)] = v
            scale = np.abs(v).max()
            gap = np.abs(r32[k].astype(np.float64) - v).max()
            out['noise_%s_%s' % (k, tag)] = np.float64(gap / scale if scale > 0 else gap)
        if tag in P.DATA_CASES:
            frac = spread_of(L, tag, case)
            assert frac[0] >= 0.1 and frac[1] >= 0.1, (tag, frac)
            out['hfrac_' + tag] = frac
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
            assert old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v), k
        print('%s reproduced: %d arrays equal' % (os.path.relpath(OUT, ROOT), len(out)))
        return
    np.savez_compressed(OUT, **out)
    print('%s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))
    for k in sorted(out):
        if k.startswith('noise_') or k.startswith('hfrac_'):
            print('  %-44s %s' % (k, out[k]))


if __name__ == '__main__':
    main()
