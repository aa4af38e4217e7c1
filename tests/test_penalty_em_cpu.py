"""CPU: the float64 restatement of the EM penalty fit (tests/penalty_em_ref.py) against the reference's recorded arrays
(tests/golden/penalty_em.npz), its bounds against deliberate mutations, and the host-side parts of arflow_amd.penalty_em."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import penalty_em_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'penalty_em.npz'), allow_pickle=False)


@pytest.fixture(scope='module')
def first_stats(gold):
    """the statistics of the first update (initial parameters), weights on: shared, never modified"""
    em = R.EMRef()
    return R.stats_ref(gold['x0'], gold['x1'], R.logw_of(em.alpha_bar, em.beta), em.beta, em.mu)


def test_fixture_inputs_are_the_seeded_ones(gold):
    x0, x1 = R.make_samples()
    assert np.array_equal(gold['x0'], x0) and np.array_equal(gold['x1'], x1) and x0.dtype == np.float32 and len(x0) == 4099
    assert np.array_equal(gold['init_vars'], np.asarray(R.INIT_VARS)) and np.array_equal(gold['lg_x'], R.log_gmm_grid())
    assert float(np.abs(gold['lg_x']).max()) == 30.0 and float(gold['lg_beta'].max()) == 1000.0
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'penalty_em.npz')) < 191444  # the smallest comparable fixture


@pytest.mark.parametrize('tag', ['w', 'u'])
def test_one_update_from_each_recorded_state(gold, tag):
    """from every recorded state one update of the restatement gives the next recorded state within update_bounds"""
    x = [gold['x0'], gold['x1'] if tag == 'w' else None]
    worst = 0.0
    for i in range(R.N_UPDATES):
        em = R.EMRef()
        if i:
            em.alpha_bar, em.beta = torch.from_numpy(gold[tag + '_alpha_bar'][i - 1]), torch.from_numpy(gold[tag + '_beta'][i - 1])
        obj = em.update(x)
        b = R.update_bounds(em)
        for key, got, bound in (('pi', em.pi, b.pi), ('alpha_bar', em.alpha_bar, b.alpha_bar), ('beta', em.beta, b.beta),
                                ('objective', obj.reshape(1), b.objective.reshape(1))):
            err = (got - torch.from_numpy(np.atleast_1d(gold['%s_%s' % (tag, key)][i]))).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (tag, i, key, float((err / bound).max()))
    print('largest error / bound over the 8 updates (%s): %.3f' % (tag, worst))


def test_trajectory_and_monotone_objective(gold):
    t = R.trajectory(gold['x0'], gold['x1'])
    ref = {k: gold['w_' + k] for k in ('pi', 'alpha_bar', 'beta', 'objective')}
    tol = float(gold['traj_margin']) * float(gold['traj_perm_dev'])
    assert 0 < float(gold['traj_perm_dev']) < 1e-12 and float(gold['traj_margin']) == 10.0
    assert R.trajectory_deviation(t, ref) <= tol
    obj = gold['w_objective']
    assert np.all(np.diff(obj) >= -tol * np.abs(obj[1:])), obj  # the reference's objective does not decrease on this input


def test_mu_sequence_matches_the_reference(gold):
    got = R.mu_sequence(R.EMRef(), [gold['x0'], gold['x1']])
    for key, v in got.items():
        assert np.all(np.isfinite(v)) and np.allclose(v, gold[key], rtol=1e-11, atol=0), key
    assert np.abs(gold['mu_ml'] - np.asarray(R.MU_START)).min() > 1e-3  # the means did move


def test_bound_holds_for_another_order_and_is_tight(gold, first_stats):
    """the same statistics summed over permuted samples sit well inside the bound; the bound itself stays small"""
    em = R.EMRef()
    p = np.random.RandomState(3).permutation(len(gold['x0']))
    other = R.stats_ref(gold['x0'][p], gold['x1'][p], R.logw_of(em.alpha_bar, em.beta), em.beta, em.mu)
    for name in ('S0', 'S1', 'S2', 'H'):
        a, b, bound = getattr(first_stats, name), getattr(other, name), getattr(first_stats, 'b' + name)
        assert bool(((a - b).abs() <= 0.25 * bound).all()), name
        scale = a.abs() if name != 'S1' else torch.as_tensor(np.abs(gold['x0']).astype(np.float64).max()) * first_stats.S0
        assert bool((bound <= 1e-11 * scale).all()), name
    assert bool((first_stats.S0 > 0).all() and (first_stats.S2 > 0).all() and (first_stats.H <= 0).all())


@pytest.mark.parametrize('mutate', R.MUTATIONS)
def test_statistics_mutations_leave_the_bound(gold, first_stats, mutate):
    em = R.EMRef()
    bad = R.stats_ref(gold['x0'], gold['x1'], R.logw_of(em.alpha_bar, em.beta, mutate), em.beta, em.mu, mutate)
    worst = 0.0
    for name in ('S0', 'S1', 'S2', 'H'):
        err = (getattr(bad, name) - getattr(first_stats, name)).abs() / getattr(first_stats, 'b' + name)
        err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
        worst = max(worst, float(err.max()))
    assert worst > 100.0, (mutate, worst)
    if mutate == 'xlogx_product':  # 0 * -inf: the product form is NaN where xi underflows; the kernel's form is finite
        assert bool(torch.isnan(bad.H).any()) and bool(torch.isfinite(first_stats.H).all())
        assert bool((first_stats.xi == 0).any())


def test_objective_with_the_new_beta_inside_xi_leaves_the_bound(gold):
    x = [gold['x0'], gold['x1']]
    good, bad = R.EMRef(), R.EMRef(mutate='new_beta_in_xi')
    og, ob = good.update(x), bad.update(x)
    bound = R.update_bounds(good).objective
    assert abs(float(og) - float(gold['w_objective'][0])) <= float(bound)
    assert abs(float(ob) - float(gold['w_objective'][0])) > 100.0 * float(bound)


def test_extreme_samples_stay_finite():
    """x = +-30 against beta = 1000: every statistic finite, H included"""
    x0 = np.asarray([30.0, -30.0, 0.0, 1e-3, 2.0], dtype=np.float32)
    beta = torch.tensor([1000.0, 1.0, 1e-3], dtype=D)
    st = R.stats_ref(x0, None, R.logw_of(torch.ones(3, dtype=D), beta), beta, torch.zeros(3, dtype=D))
    for name in ('S0', 'S1', 'S2', 'H', 'bS0', 'bS1', 'bS2', 'bH'):
        assert bool(torch.isfinite(getattr(st, name)).all()), name
    assert float(st.xi[0, 0]) == 0.0


def test_log_gmm_restatement_matches_the_reference_and_finite_differences(gold):
    x = torch.from_numpy(gold['lg_x']).to(D)
    out, grad, c, gabs = R.log_gmm_ref(x, gold['lg_pi'], gold['lg_beta'])
    bo, bg = R.log_gmm_bounds(out, c, gabs, D)
    assert bool(((out - torch.from_numpy(gold['lg_out'])).abs() <= bo).all())
    assert bool(((grad - torch.from_numpy(gold['lg_grad'])).abs() <= bg + 1e-300).all())
    h = 1e-6 * (1 + x.abs())
    fd = (R.log_gmm_ref(x + h, gold['lg_pi'], gold['lg_beta'])[0] - R.log_gmm_ref(x - h, gold['lg_pi'], gold['lg_beta'])[0]) / (2 * h)
    assert bool(((fd - grad).abs() <= 1e-6 * (1 + grad.abs())).all())


def test_launch_geometry_mirror_matches_the_library():
    from arflow_amd import _lib, penalty_em as P
    lib = _lib.load()
    for m in (1, 63, 1023, 1024, 1025, 4099, 1024 * 1024, 1024 * 1024 + 1, 3000000):
        assert lib.arflow_em_partials(m) == R.partials(m), m
        assert P.em_share(m) == R.share(m)
    assert R.partials(4099) == 5 and R.share(3000000) == 3072 and R.partials(3000000) <= 1024
    assert lib.arflow_em_partials(0) == -1002


def test_argument_errors_without_gpu():
    from arflow_amd import _lib
    lib = _lib.load()
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)
    assert lib.arflow_em_stats(None, None, 8, 0, one, one, one, 3, one, None) == -1001
    assert lib.arflow_em_stats(one, None, 0, 0, one, one, one, 3, one, None) == -1002
    assert lib.arflow_em_stats(one, None, 8, 0, one, one, one, 17, one, None) == -1003
    assert lib.arflow_em_stats(one, None, 8, 0, one, one, one, 0, one, None) == -1003
    assert lib.arflow_em_stats(one, None, 8, 2, one, one, one, 3, one, None) == -1003
    assert lib.arflow_em_stats(odd, None, 8, 1, one, one, one, 3, one, None) == -1003  # float64 samples off an 8-byte boundary
    assert lib.arflow_em_fold(one, 0, 3, one, None) == -1002 and lib.arflow_em_fold(one, 1025, 3, one, None) == -1002
    assert lib.arflow_log_gmm_fwd(one, 0, 0, one, one, 3, one, None) == -1002
    assert lib.arflow_log_gmm_fwd(one, 4, 0, one, one, 17, one, None) == -1003
    assert lib.arflow_log_gmm_bwd(one, None, 4, 0, one, one, 3, one, None) == -1001
    assert lib.arflow_census_residual(one, one, one, one, None, 1, 8, 8, 3, None) == -1001
    assert lib.arflow_census_residual(one, one, one, one, one, 1, 8, 8, 4, None) == -1003
    assert lib.arflow_census_residual(one, one, one, one, one, 0, 8, 8, 3, None) == -1002


def test_fwhm_scale_and_widths(gold):
    from arflow_amd import penalty_em as P
    assert P.robust_l1_fwhm() == float(gold['fwhm_robust_l1']) and P.abs_robust_loss_fwhm() == float(gold['fwhm_abs_robust'])
    k = len(R.INIT_VARS)
    root = P.fwhm_scale(gold['w_pi'][-1], np.zeros(k), gold['w_beta'][-1], P.robust_l1_fwhm())
    # scipy's bisection stops at xtol = 2e-12 (its default); ours runs until the bracket no longer shrinks
    assert abs(root - float(gold['fwhm_root'])) <= 4e-12
    half = P.gaussian_mixture(np.array([P.robust_l1_fwhm() / 2, 0.0]), gold['w_pi'][-1], np.zeros(k), root * gold['w_beta'][-1])
    assert abs(half[0] / half[1] - 0.5) < 1e-12
    with pytest.raises(ValueError):
        P.fwhm_scale([1.0], [0.0], [1.0], 1e-9)  # the half width is never reached on the bracket


def test_collect_samples_restates_the_scripts_loop(gold):
    """pure torch: runs on the CPU.  Against an independent numpy statement of the loop on the recorded smoothness terms."""
    from arflow_amd import penalty_em as P
    losses = [torch.from_numpy(gold['smooth_x'])[:, :, :, 0:-1].float(), torch.from_numpy(gold['smooth_y'])[:, :, 0:-1, :].float()]
    weights = [torch.from_numpy(gold['smooth_wx'])[:, :, :, 0:-1].repeat([1, 2, 1, 1]).float(),
               torch.from_numpy(gold['smooth_wy'])[:, :, 0:-1, :].repeat([1, 2, 1, 1]).float()]
    weights[0][0, :, 0, 0] = 0.0  # an entry the 1e-6 rule drops whatever its draw
    rand = R.collect_rand([w.shape for w in weights])
    x = P.collect_samples(losses, weights, R.SUBSAMPLE, rand=rand)
    want = []
    for l, w, r in zip(losses, weights, rand):
        l, w, r = l.numpy(), w.numpy(), r.numpy()
        keep = ((w / w.max()) > 1e-6) & (r > R.SUBSAMPLE)
        want.append(l[keep])
    want = np.concatenate(want)
    assert x.shape == (2, len(want)) and 0.3 * losses[0].numel() < len(want) < 1.7 * losses[0].numel()
    assert np.array_equal(x[0].numpy(), want) and bool((x[1] == 1).all())
    keep0 = (rand[0] > R.SUBSAMPLE).sum() - (rand[0][0, :, 0, 0] > R.SUBSAMPLE).sum()
    assert int(keep0) + int((rand[1] > R.SUBSAMPLE).sum()) == len(want)


def test_em_refuses_cpu_tensors_and_bad_k():
    from arflow_amd import _lib, penalty_em as P
    with pytest.raises(_lib.ArflowHipError):
        P.EM(k=2, init_vars=[1.0, 2.0], device='cpu')
    with pytest.raises(ValueError):
        P.EM(k=17, init_vars=[1.0] * 17, device='cuda')
    with pytest.raises(_lib.ArflowHipError):
        P.log_gmm(torch.zeros(3), [1.0], [1.0])
    with pytest.raises(NotImplementedError, match='mean'):
        P.data_loss_no_penalty(None, None, None, None, 'mean', ['census'])
    with pytest.raises(NotImplementedError, match='ssim'):
        P.data_loss_no_penalty(None, None, None, None, 'sample', ['ssim'])
