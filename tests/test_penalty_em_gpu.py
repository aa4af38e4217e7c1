"""GPU: the one-pass EM statistics, the EM class built on them, log_gmm and the residual collection (csrc/penalty_em.hip,
arflow_census_residual in csrc/photo.hip, arflow_amd/penalty_em.py) against the float64 restatement of tests/penalty_em_ref.py
and the reference's recorded arrays (tests/golden/penalty_em.npz).  DESIGN.md section 44.

Every bound comes from tests/penalty_em_ref.py (derived from the inputs; tests/test_penalty_em_cpu.py shows that the listed
mutations leave it by > 100x) or from tests/census_ref.py for the census distance.  Each test prints its largest error / bound.
Sample counts: 1, 63, 64, 65 (one wave and its neighbours), 1023 / 1024 / 1025 (one workgroup's share and its neighbours), 4099
(five workgroups, the last with a ragged tail of 3 samples); k = 1, 10 (K <= 16 kernel, six idle slots), 16, and k = 8 (the
K <= 8 kernel, full) at 4099.

Tolerances of the residual collection against the float64 fixture (the product computes in fp32 what the reference computed in
float64; u = 2^-24):
  warped image   the sampling coordinate carries the x4 upsample of the flow (4 u 4 |flow|, |flow| <= 3) and the fp32 normalise /
                 un-normalise round trip (6 u W): <= 1.5e-5 px at W = 24; the images lie in [0, 1], so neighbouring pixels differ
                 by at most 1: d img <= 1.5e-5 + 5 u (the blend).  Grey plane: 255 (d img + 6 u).  Through census_ref.census_core.
  masks          mask_invalid is a comparison: equal unless a coordinate lies within 1.5e-5 px of the border (none does on the
                 seeded input: asserted exactly).  Range map: four splat weights, each a product of two fp32 differences of a
                 coordinate with error 2 u |coord|: <= 1e-5 after the clamp and the x4 blend; the weight divides by the sum of
                 the same terms: rtol 2e-5, atol 1e-5 / sum.
  smoothness     a difference of two fp32 numbers rounds once (rtol u);  the edge weight is exp(-mean |150 g|) / 2 with g a
                 difference of 2 x 2 means of the image (4 u each): exponent error <= 150 x 8 u, weight <= 1 / 2: atol 5e-5.
"""
import numpy as np
import pytest
import torch

from arflow_amd import functional as AF
from arflow_amd import penalty_em as P
from arflow_amd import uflow_utils as UU
from tests import census_ref as C
from tests import penalty_em_ref as R
from tests.loss_kernels_ref import worst

pytestmark = pytest.mark.gpu
DEV = 'cuda'
D = torch.float64
_cache = {}


def gold(golden):
    return golden('penalty_em')


def mixture(k, seed, zero_mu=False):
    """seeded alpha_bar, beta (spanning 1e-2 .. 1e3), mu of a k-component state, float64 CPU"""
    g = torch.Generator().manual_seed(100 + 17 * k + seed)
    alpha_bar = 1 + 50 * torch.rand(k, generator=g, dtype=D)
    beta = 10 ** (-2 + 5 * torch.rand(k, generator=g, dtype=D))
    mu = torch.zeros(k, dtype=D) if zero_mu else 0.3 * torch.randn(k, generator=g, dtype=D)
    return alpha_bar, beta, mu


def check_stats(x0, x1, alpha_bar, beta, mu, what):
    """arflow_em_stats + arflow_em_fold on (x0, x1) against stats_ref within its bounds; -> largest error / bound"""
    logw = R.logw_of(alpha_bar, beta)
    ref = R.stats_ref(x0, x1, logw, beta, mu)
    dx0 = torch.as_tensor(x0).to(DEV)
    dx1 = None if x1 is None else torch.as_tensor(x1).to(DEV)
    part = P.em_partials(dx0, dx1, logw.to(DEV), beta.to(DEV), mu.to(DEV))
    stats = P.em_stats(dx0, dx1, logw.to(DEV), beta.to(DEV), mu.to(DEV)).cpu()
    assert part.shape == (R.partials(len(x0)), 4, len(beta)) and bool(torch.isfinite(part).all()), what
    assert bool(torch.isfinite(stats).all()), what
    fold = torch.zeros(4, len(beta), dtype=D)
    for b in range(part.shape[0]):  # the fold kernel's order, on the host
        fold = fold + part[b].cpu()
    assert torch.equal(fold, stats), what
    w = 0.0
    for i, name in enumerate(('S0', 'S1', 'S2', 'H')):
        r = worst((stats[i] - getattr(ref, name)).abs(), getattr(ref, 'b' + name))
        assert r <= 1.0, '%s: %s off by %.3g bounds' % (what, name, r)
        w = max(w, r)
    return w


@pytest.mark.parametrize('k', [1, 10, 16])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_statistics_within_bound(m, k):
    x0, x1 = R.make_samples(m, seed=m)
    z = x1.copy()
    z[::3] = 0.0
    w = 0.0
    for dt in (np.float32, np.float64):
        # unit weights with zero means; weights and weights with zeros with non-zero means
        w = max(w, check_stats(x0.astype(dt), None, *mixture(k, 0, zero_mu=True), what='%s null' % dt.__name__))
        w = max(w, check_stats(x0.astype(dt), x1.astype(dt), *mixture(k, 1), what='%s weights' % dt.__name__))
        w = max(w, check_stats(x0.astype(dt), z.astype(dt), *mixture(k, 2), what='%s zeros' % dt.__name__))
    print('m = %d, k = %d: largest error / bound %.3f' % (m, k, w))


def test_statistics_k8_kernel_and_float64_detail():
    """k = 8 fills the K <= 8 instantiation; float64 samples that are not fp32 numbers"""
    x0, x1 = R.make_samples(4099, seed=8)
    x64 = x0.astype(np.float64) * (1 + 1e-9)
    w = max(check_stats(x0, x1, *mixture(8, 3), what='k8 f32'), check_stats(x64, x1.astype(np.float64), *mixture(8, 4), what='k8 f64'))
    print('k = 8: largest error / bound %.3f' % w)


@pytest.mark.parametrize('k', [3, 10])
def test_extreme_samples_stay_finite(k):
    """x = +-30 against beta = 1000: no NaN or inf anywhere, H finite and within its bound"""
    x0 = np.concatenate([R.make_samples(70, seed=5)[0], np.asarray([30.0, -30.0, 0.0, 29.5], dtype=np.float32)])
    alpha_bar, beta, mu = mixture(k, 5, zero_mu=True)
    beta[0], beta[-1] = 1000.0, 1e-3
    w = max(check_stats(x0, None, alpha_bar, beta, mu, 'extreme'),
            check_stats(x0.astype(np.float64), None, alpha_bar, beta, mu + 0.25, 'extreme mu'))
    print('extreme, k = %d: largest error / bound %.3f' % (k, w))


def test_two_calls_give_the_same_bits():
    x0, x1 = (torch.from_numpy(t).to(DEV) for t in R.make_samples())
    alpha_bar, beta, mu = (t.to(DEV) for t in mixture(10, 6))
    logw = R.logw_of(alpha_bar.cpu(), beta.cpu()).to(DEV)
    parts = []
    for det in (False, True, False):
        prev = AF.set_deterministic(det)
        try:
            parts.append(P.em_partials(x0, x1, logw, beta, mu).view(torch.int64).cpu())
        finally:
            AF.set_deterministic(prev)
    assert torch.equal(parts[0], parts[1]) and torch.equal(parts[0], parts[2])


def product_em(state=None):
    em = P.EM(k=len(R.INIT_VARS), init_vars=R.INIT_VARS, device=DEV)
    if state is not None:
        em.alpha_bar, em.beta = (torch.as_tensor(t, dtype=D).to(DEV) for t in state)
    return em


@pytest.mark.parametrize('tag', ['w', 'u'])
def test_one_update_from_each_recorded_state(golden, tag):
    z = gold(golden)
    x0, x1 = z.raw('x0'), z.raw('x1')
    dx = [torch.from_numpy(x0).to(DEV), torch.from_numpy(x1).to(DEV) if tag == 'w' else None]
    w = 0.0
    for i in range(R.N_UPDATES):
        state = None if i == 0 else (z.raw(tag + '_alpha_bar')[i - 1], z.raw(tag + '_beta')[i - 1])
        em, ref = product_em(state), R.EMRef()
        if state is not None:
            ref.alpha_bar, ref.beta = torch.from_numpy(state[0]), torch.from_numpy(state[1])
        obj = em.update(dx)
        ref.update([x0, x1 if tag == 'w' else None])
        b = R.update_bounds(ref)
        assert em.xi is None
        for key, got, bound in (('pi', em.pi, b.pi), ('alpha_bar', em.alpha_bar, b.alpha_bar), ('beta', em.beta, b.beta),
                                ('objective', obj.reshape(1), b.objective.reshape(1))):
            want = torch.from_numpy(np.atleast_1d(z.raw('%s_%s' % (tag, key))[i]))
            r = worst((got.cpu() - want).abs(), bound)
            assert r <= 1.0, 'update %d (%s): %s off by %.3g bounds' % (i, tag, key, r)
            w = max(w, r)
    print('one update from each recorded state (%s): largest error / bound %.3f' % (tag, w))


def test_trajectory_of_eight_updates(golden):
    z = gold(golden)
    tol = float(z.raw('traj_margin')) * float(z.raw('traj_perm_dev'))
    x = [torch.from_numpy(z.raw('x0')).to(DEV), torch.from_numpy(z.raw('x1')).to(DEV)]
    em, obj = product_em(), []
    for _ in range(R.N_UPDATES):
        obj.append(em.update(x))
    obj = torch.stack(obj).cpu().numpy()
    got = {'pi': em.pi.cpu().numpy()[None], 'beta': em.beta.cpu().numpy()[None], 'objective': obj[-1:]}
    ref = {k: z.raw('w_' + k) for k in ('pi', 'beta', 'objective')}
    dev = R.trajectory_deviation(got, ref)
    print('relative deviation after 8 updates %.3e (allowed %.3e = 10 x the permutation figure)' % (dev, tol))
    assert dev <= tol
    assert np.all(np.diff(obj) >= -tol * np.abs(obj[1:])), obj
    pi, mu, beta, objs = P.fit_penalty(x[0], x[1], R.INIT_VARS, n_iter=R.N_UPDATES)
    assert torch.equal(pi, em.pi) and torch.equal(beta, em.beta) and torch.equal(objs.cpu(), torch.from_numpy(obj))
    assert bool((mu == 0).all()) and objs.shape == (R.N_UPDATES,)
    root = P.fwhm_scale(pi, mu, beta, P.robust_l1_fwhm())
    assert abs(root - float(z.raw('fwhm_root'))) <= 1e-10 * root  # the root moves with pi and beta (1e-14 relative), first order


def test_mu_sequence_matches_the_reference(golden):
    """update_mu_ml / update_mu_map from a non-zero mu: S2 is re-centred by the identity, not by another pass"""
    z = gold(golden)
    x = [torch.from_numpy(z.raw('x0')).to(DEV), torch.from_numpy(z.raw('x1')).to(DEV)]
    got = R.mu_sequence(product_em(), x)
    for key, v in got.items():
        assert np.all(np.isfinite(v)) and np.allclose(v, z.raw(key), rtol=1e-11, atol=0), key
    em = product_em()
    em.mu = torch.as_tensor(R.MU_START, dtype=D).to(DEV)
    xi = em.responsibilities(x)
    em.update_xi(x)
    assert np.allclose((xi * x[1].double()[:, None]).sum(0).cpu().numpy(), em.S0.cpu().numpy(), rtol=1e-12)


LG_SHAPES = ['one', 'n65', 'view4d', 'grid']


def lg_input(shape, golden):
    g = torch.Generator().manual_seed(21)
    if shape == 'one':
        return torch.tensor([0.37])
    if shape == 'n65':
        return 6 * torch.randn(65, generator=g)
    if shape == 'view4d':
        return (4 * torch.randn(2, 3, 5, 14, generator=g))[:, 1:3, :, ::2]  # non-contiguous [2, 2, 5, 7]
    return torch.from_numpy(gold(golden).raw('lg_x'))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('shape', LG_SHAPES)
def test_log_gmm_forward_and_gradient(golden, shape, dtype):
    z = gold(golden)
    pi, beta = z.raw('lg_pi'), z.raw('lg_beta')
    base = lg_input(shape, golden).to(dtype)
    storage = base.to(DEV) if shape != 'view4d' else None
    if shape == 'view4d':
        full = (4 * torch.randn(2, 3, 5, 14, generator=torch.Generator().manual_seed(21))).to(dtype).to(DEV)
        x = full[:, 1:3, :, ::2]
        assert not x.is_contiguous() and torch.equal(x.cpu(), base)
    else:
        x = storage
    x = x.detach().requires_grad_(True)
    out = P.log_gmm(x, pi, beta)
    gup = torch.linspace(0.5, 1.5, base.numel(), dtype=dtype).reshape(base.shape)
    out.backward(gup.to(DEV))
    ro, rg, c, gabs = R.log_gmm_ref(base, pi, beta)
    bo, bg = R.log_gmm_bounds(ro, c, gabs, dtype)
    assert out.shape == base.shape and out.dtype == dtype and x.grad.shape == base.shape
    w = max(worst((out.detach().cpu().double() - ro).abs(), bo),
            worst((x.grad.cpu().double() - rg * gup.double()).abs(), bg * gup.double() + 2 * torch.finfo(dtype).eps * (rg * gup).abs()))
    print('log_gmm %s %s: largest error / bound %.3f' % (shape, dtype, w))
    assert w <= 1.0
    if shape == 'grid':  # the reference's own values and autograd gradient
        assert worst((out.detach().cpu().double() - torch.from_numpy(z.raw('lg_out'))).abs(), 2 * bo) <= 1.0
        assert worst((x.grad.cpu().double() - torch.from_numpy(z.raw('lg_grad')) * gup.double()).abs(),
                     2 * bg * gup.double() + 4 * torch.finfo(dtype).eps * (rg * gup).abs()) <= 1.0
    if dtype == torch.float64:  # central differences of the float64 restatement
        h = 1e-6 * (1 + base.abs())
        fd = (R.log_gmm_ref(base + h, pi, beta)[0] - R.log_gmm_ref(base - h, pi, beta)[0]) / (2 * h)
        assert bool(((fd * gup - x.grad.cpu()).abs() <= 1e-6 * (1 + (rg * gup).abs())).all())


def census_case(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g),
            (torch.rand(B, 1, H, W, generator=g) > 0.3).float())


def check_census(im_a, im_b, mask, what):
    ham, wgt = UU.census_loss_no_penalty(im_a.to(DEV), im_b.to(DEV), mask.to(DEV))
    ref = C.standalone_ref(im_a, im_b, 3, mask=mask)
    assert ham.shape == mask.shape and wgt.shape == mask.shape and not ham.requires_grad
    r = worst((ham.cpu().double() - ref.ham).abs(), ref.ham_bound)
    want = ref.pm / (ref.pm.sum() + 1e-6)
    r2 = worst((wgt.cpu().double() - want).abs(), 8 * C.U * want)  # 0 / 1 terms: an exact fp32 sum; + 1e-6, the quotient
    assert r <= 1.0 and r2 <= 1.0, (what, r, r2)
    return max(r, r2)


@pytest.mark.parametrize('shape', [(2, 9, 13), (1, 12, 16), (2, 19, 45)])
def test_census_residual_per_pixel(shape):
    """9 x 13: W % 4 != 0, smaller than a tile; 12 x 16; 19 x 45: more than one 8 x 32 tile in both directions"""
    im_a, im_b, mask = census_case(*shape, seed=sum(shape))
    w = check_census(im_a, im_b, mask, shape)
    ham, _ = UU.census_loss_no_penalty(im_a.to(DEV), im_a.to(DEV), mask.to(DEV))
    assert bool((ham == 0).all())  # an image against itself: exactly 0 (in the interior and in the zero padding)
    print('census residual %s: largest error / bound %.3f' % (shape, w))
    with pytest.raises(ValueError, match='fused loss paths'):
        UU.census_loss_no_penalty(im_a.to(DEV).requires_grad_(True), im_b.to(DEV), mask.to(DEV))


def residuals(golden):
    if 'res' not in _cache:
        z = gold(golden)
        _cache['res'] = {k: torch.from_numpy(z.raw('res_' + k)) for k in ('im1', 'im2', 'flow12', 'flow21', 'mask')}
    return _cache['res']


def test_census_residual_against_the_fixture(golden):
    z, res = gold(golden), residuals(golden)
    w = check_census(res['im1'], res['im2'], res['mask'], 'fixture')
    ham, wgt = UU.census_loss_no_penalty(res['im1'].to(DEV), res['im2'].to(DEV), res['mask'].to(DEV))
    ref = C.standalone_ref(res['im1'], res['im2'], 3, mask=res['mask'])
    assert worst((ham.cpu().double() - torch.from_numpy(z.raw('census_ham'))).abs(), ref.ham_bound) <= 1.0
    assert np.allclose(wgt.cpu().numpy(), z.raw('census_weight'), rtol=8 * C.U, atol=0)
    print('census residual fixture: largest error / bound %.3f' % w)


@pytest.mark.parametrize('occ', ['sample', 'none'])
def test_data_loss_no_penalty_against_the_fixture(golden, occ):
    z, res = gold(golden), residuals(golden)
    loss, weight, occu, valid = P.data_loss_no_penalty(*(res[k].to(DEV) for k in ('im1', 'im2', 'flow12', 'flow21')), occ, ['census'])
    assert len(loss) == 1 and len(weight) == 1
    assert torch.equal(valid.cpu().double(), torch.from_numpy(z.raw('data_%s_valid' % occ)))
    # the warped image in float64, for the bound only: grey error 255 (1.5e-5 + 5 u + 6 u) (the module docstring)
    f0 = torch.nn.functional.interpolate(res['flow12'].double(), scale_factor=4.0, mode='bilinear', align_corners=False) * 4.0
    B, _, H, W = f0.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D), torch.arange(W, dtype=D), indexing='ij')
    grid = torch.stack([2 * (xs + f0[:, 0]) / (W - 1) - 1, 2 * (ys + f0[:, 1]) / (H - 1) - 1], dim=-1)
    rec = torch.nn.functional.grid_sample(res['im2'].double(), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    core = C.census_core(C.gray255_ref(res['im1']), C.gray255_ref(rec), 3, 6 * C.U * 255.0, 255.0 * (1.5e-5 + 11 * C.U))
    want = torch.from_numpy(z.raw('data_%s_loss' % occ))
    assert float((core.ham - want).abs().max()) <= 1e-9  # the bound's own warp is the reference's
    r = worst((loss[0].cpu().double() - want).abs(), core.ham_bound)
    wref = torch.from_numpy(z.raw('data_%s_weight' % occ))
    total = float(torch.from_numpy(z.raw('data_%s_weight' % occ)).gt(0).sum())
    r2 = worst((weight[0].cpu().double() - wref).abs(), 2e-5 * wref + 1e-5 / max(total, 1.0))
    if occ == 'sample':
        assert float((occu.cpu().double() - torch.from_numpy(z.raw('data_sample_occu'))).abs().max()) <= 1e-5
    else:
        assert occu is None
    print('data_loss_no_penalty %s: largest error / bound loss %.3f weight %.3f' % (occ, r, r2))
    assert r <= 1.0 and r2 <= 1.0
    with pytest.raises(NotImplementedError, match='mean'):
        P.data_loss_no_penalty(None, None, None, None, 'mean', ['census'])


def test_smooth_loss_and_collect_samples_against_the_fixture(golden):
    z, res = gold(golden), residuals(golden)
    sx, wx, sy, wy = P.smooth_loss_no_penalty(res['im1'].to(DEV), res['flow12'].to(DEV), R.EDGE_CONSTANT, R.EDGE_ASYMP)
    for got, key, rtol, atol in ((sx, 'smooth_x', 2 * C.U, 0.0), (sy, 'smooth_y', 2 * C.U, 0.0), (wx, 'smooth_wx', 0.0, 5e-5),
                                 (wy, 'smooth_wy', 0.0, 5e-5)):
        want = z.raw(key)
        assert got.shape == want.shape and np.allclose(got.cpu().numpy(), want, rtol=rtol, atol=atol), key
    # the script's lists for the forward direction (train_penalty_em.py:268-270), a seeded draw per entry
    losses = [sx[:, :, :, 0:-1], sy[:, :, 0:-1, :]]
    weights = [wx[:, :, :, 0:-1].repeat([1, 2, 1, 1]), wy[:, :, 0:-1, :].repeat([1, 2, 1, 1])]
    rand = R.collect_rand([w.shape for w in weights])
    x = P.collect_samples(losses, weights, R.SUBSAMPLE, rand=rand)
    want = np.concatenate([l.cpu().numpy()[((w / w.max()).cpu().numpy() > 1e-6) & (r.numpy() > R.SUBSAMPLE)]
                           for l, w, r in zip(losses, weights, rand)])
    assert x.shape == (2, len(want)) and 20 < len(want) < losses[0].numel() + losses[1].numel() and x.is_cuda
    assert np.array_equal(x[0].cpu().numpy(), want) and bool((x[1] == 1).all())
    pi, mu, beta, obj = P.fit_penalty(x[0], x[1], n_iter=3)  # the collected samples feed the fit as they are
    assert bool(torch.isfinite(obj).all()) and abs(float(pi.sum()) - 1) < 1e-12
