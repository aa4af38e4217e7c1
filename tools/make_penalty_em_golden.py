#!/usr/bin/env python3
"""tests/golden/penalty_em.npz: the seeded inputs of tests/penalty_em_ref.py and what the REFERENCE's own code makes of them --
class EM and the FWHM helpers of train_penalty_em.py, log_gmm / data_loss_no_penalty / smooth_loss_no_penalty of
losses/uflow_elbo_loss.py, census_loss_no_penalty of utils/uflow_utils.py, all imported live -- on the CPU with float64 as the
default dtype.

    python tools/make_penalty_em_golden.py --reference /path/to/reference [--check]

train_penalty_em.py imports easydict, datasets.get_dataset and losses.get_loss at its top (the latter pulls in cv2); where one
does not import, an empty stand-in module is registered: the script's body is under __main__ and nothing here touches them.
  x0, x1 [4099] fp32, init_vars           the samples (three scales), the weights in [0.1, 1.1), the script's init_vars
  w_pi, w_alpha_bar, w_beta [8, k], w_objective [8]     after each of 8 EM.update() calls with the weights;  u_*: with x1 = 1
  mu_ml, beta_ml, obj_ml, mu_map, beta_map, obj_map     penalty_em_ref.mu_sequence on the reference's EM (weights on)
  lg_x fp32, lg_pi, lg_beta, lg_out, lg_grad            log_gmm on the float64 grid and its autograd gradient
  res_im1, res_im2, res_flow12, res_flow21, res_mask    the seeded 16 x 24 pair, its 4 x 6 flows, a seeded mask
  census_ham, census_weight                              census_loss_no_penalty(im1, im2, mask)
  data_sample_loss / _weight / _occu / _valid            data_loss_no_penalty(.., 'sample', ['census'])
  data_none_loss / _weight / _valid                      occ_type 'none': the reference's function ends in a return statement that
                                                         names two variables this branch never binds (UnboundLocalError, asserted
                                                         here), so its lines for that branch (:33-38, :60, :71) are run one by one
                                                         on the reference's own upsample / flow_to_warp / resample / mask_invalid /
                                                         census_loss_no_penalty
  smooth_x, smooth_wx, smooth_y, smooth_wy               smooth_loss_no_penalty(im1, flow12, 150, 0.01)
  fwhm_robust_l1, fwhm_abs_robust, fwhm_root             the script's two reference widths; scipy's root_scalar(bisect, [1e-6, 100])
                                                         of the script's function for (w_pi[-1], 0, w_beta[-1]) and robust_l1's width
  traj_perm_dev, traj_margin                             penalty_em_ref.permutation_deviation (the float64 RESTATEMENT under 8
                                                         seeded sample permutations, weights on) and the factor the GPU test allows
--check regenerates in memory and compares with the committed file instead of writing it.  Arrays only.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import penalty_em_ref as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'penalty_em.npz')
TRAJ_MARGIN = 10.0


def reference_modules(reference_root):
    sys.path.insert(0, reference_root)
    import matplotlib
    matplotlib.use('Agg')
    import losses.uflow_elbo_loss as L
    import utils.uflow_utils as UU
    for name, attrs in (('easydict', ('EasyDict',)), ('datasets', ()), ('datasets.get_dataset', ('get_dataset',)),
                        ('losses.get_loss', ('get_loss',))):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            for a in attrs:
                setattr(mod, a, None)
            sys.modules[name] = mod
    import train_penalty_em as T
    for mod in (L, UU, T):
        assert os.path.abspath(mod.__file__).startswith(reference_root), mod.__file__
    return T, L, UU


def run_updates(T, x, init_vars):
    em = T.EM(k=len(init_vars), init_vars=init_vars)
    rec = {'pi': [], 'alpha_bar': [], 'beta': [], 'objective': []}
    for _ in range(R.N_UPDATES):
        obj = em.update(x)
        for key, v in (('pi', em.pi), ('alpha_bar', em.alpha_bar), ('beta', em.beta), ('objective', obj)):
            rec[key].append(v.clone().numpy())
    return {key: np.stack(v) for key, v in rec.items()}


def generate(reference_root):
    torch.set_default_dtype(torch.float64)
    T, L, UU = reference_modules(reference_root)
    x0, x1 = R.make_samples()
    out = {'x0': x0, 'x1': x1, 'init_vars': np.asarray(R.INIT_VARS, dtype=np.float64)}
    tx0, tx1 = torch.from_numpy(x0).double(), torch.from_numpy(x1).double()
    for tag, x in (('w', [tx0, tx1]), ('u', [tx0, torch.ones_like(tx0)])):
        for key, v in run_updates(T, x, R.INIT_VARS).items():
            out['%s_%s' % (tag, key)] = v
    out.update(R.mu_sequence(T.EM(k=len(R.INIT_VARS), init_vars=R.INIT_VARS), [tx0, tx1]))

    g = torch.from_numpy(R.log_gmm_grid()).double().requires_grad_(True)
    lg = L.log_gmm(g, R.LG_PI, R.LG_BETA)
    lg.sum().backward()
    out.update(lg_x=R.log_gmm_grid(), lg_pi=np.asarray(R.LG_PI), lg_beta=np.asarray(R.LG_BETA), lg_out=lg.detach().numpy(),
               lg_grad=g.grad.numpy())

    res = R.residual_inputs()
    B, H, W = R.RES_SHAPE
    mask = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float32) > 0.2).float()
    assert all(v.dtype == torch.float32 for v in res.values()) and mask.dtype == torch.float32
    out.update({'res_' + k: v.numpy() for k, v in res.items()}, res_mask=mask.numpy())
    im1, im2, f12, f21 = (res[k].double() for k in ('im1', 'im2', 'flow12', 'flow21'))
    ham, wgt = UU.census_loss_no_penalty(im1, im2, mask.double())
    out.update(census_ham=ham.numpy(), census_weight=wgt.numpy())
    loss, wt, occu, valid = L.data_loss_no_penalty(im1, im2, f12, f21, 'sample', ['census'])
    out.update(data_sample_loss=loss[0].numpy(), data_sample_weight=wt[0].numpy(), data_sample_occu=occu.numpy(),
               data_sample_valid=valid.numpy())
    try:
        L.data_loss_no_penalty(im1, im2, f12, f21, 'none', ['census'])
        raise AssertionError('the reference returns for occ_type none: record its own return value instead')
    except UnboundLocalError:
        pass
    warp12_0 = UU.flow_to_warp(UU.upsample(f12.clone(), is_flow=True, scale_factor=4.0))
    mask_0 = torch.detach(UU.mask_invalid(warp12_0))
    l, w = UU.census_loss_no_penalty(im1, UU.resample(im2.detach(), warp12_0), mask_0)
    out.update(data_none_loss=l.numpy(), data_none_weight=w.numpy(), data_none_valid=mask_0.numpy())
    sx, swx, sy, swy = L.smooth_loss_no_penalty(im1, f12, R.EDGE_CONSTANT, R.EDGE_ASYMP)
    out.update(smooth_x=sx.numpy(), smooth_wx=swx.numpy(), smooth_y=sy.numpy(), smooth_wy=swy.numpy())

    pi, beta, mu = out['w_pi'][-1], out['w_beta'][-1], np.zeros(len(R.INIT_VARS))
    fwhm = T.robust_l1_fwhm()
    from scipy.optimize import root_scalar

    def func(a):
        return T.gaussian_mixture(np.array([fwhm / 2]), pi, mu, a * beta) - T.gaussian_mixture(np.array([0]), pi, mu, a * beta) / 2
    sol = root_scalar(func, method='bisect', bracket=[1e-6, 100])
    out.update(fwhm_robust_l1=np.float64(fwhm), fwhm_abs_robust=np.float64(T.abs_robust_loss_fwhm()), fwhm_root=np.float64(sol.root))
    out.update(traj_perm_dev=np.float64(R.permutation_deviation(x0, x1)), traj_margin=np.float64(TRAJ_MARGIN))
    return {k: np.asarray(v) for k, v in out.items()}


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
    print('%s: %d bytes, %d arrays; trajectory deviation under permutation %.3e' %
          (os.path.relpath(OUT, ROOT), os.path.getsize(OUT), len(out), float(out['traj_perm_dev'])))


if __name__ == '__main__':
    main()
