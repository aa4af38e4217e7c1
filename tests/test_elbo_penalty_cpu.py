"""CPU: the selectable penalties and mean-flow masks of UFlowElboLoss without a GPU -- the float64
restatement of tests/elbo_penalty_ref.py against what the reference's own loss computed (tests/golden/elbo_penalty.npz), the
mutations that must leave the bounds, the penalty pairs and their error bounds, the constructor's validation, the argument
errors of the new entry points and the penalty_cfg round trip.

Measured here (printed by the tests): the restatement meets every golden array with error / bound <= 0.05 (largest 1.3e-10:
both are float64 runs of the same arithmetic); each mutation must leave its case's bound by more than 100x, the margin
tests/census_ref.py asks of its own -- the smallest ratio measured is 1.66e4 (gmm_sq_on_distance on gmm_data; then 6.1e4
gmm_on_squared_difference, 1.6e5 mean_range_map_from_sample, 2.8e5 weights_without_sqrt_beta, 5.0e5
mean_validity_from_sample, 7.1e5 charbonnier_on_h_squared).  Plain fp32 torch arithmetic in the kernels' order sits inside
the penalty bounds with 2x room (largest error / bound 0.33, CHARBONNIER)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import elbo_penalty_ref as P
from tests import elbo_ref as R


def _case(g, tag):
    kind = P.CASES[tag]['inputs']
    case = {k: g.raw('%s_%s' % (k, tag)) for k in ('net12', 'net21', 'eps12', 'eps21')}
    case.update(im1=g.raw('im1_' + kind), im2=g.raw('im2_' + kind))
    return case


def _worst_ratio(g, tag, got):
    worst = {}
    for key in P.OUTPUTS:
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        worst[key] = float((np.abs(got[key] - ref) / P.golden_bound(g, key, tag)).max())
    return worst


@pytest.fixture(scope='module')
def restated(golden):
    g = golden('elbo_penalty')
    return {tag: P.loss(P.case_cfg(tag), _case(g, tag)) for tag in P.CASES}


def test_the_fixture_holds_the_recipe(golden):
    g = golden('elbo_penalty')
    for tag in P.CASES:
        case = P.make_case(tag)
        for k, v in _case(g, tag).items():
            assert np.array_equal(v, case[k]), (tag, k)
    for tag in P.DATA_CASES:  # the census distances spread over the mixture's components
        lo, hi = g.raw('hfrac_' + tag)
        assert lo >= 0.1 and hi >= 0.1, (tag, lo, hi)


@pytest.mark.parametrize('tag', list(P.CASES))
def test_restatement_meets_the_reference(golden, restated, tag):
    g = golden('elbo_penalty')
    worst = _worst_ratio(g, tag, restated[tag])
    print(tag, {k: '%.2e' % v for k, v in worst.items()})
    assert max(worst.values()) <= 0.05, worst
    cfg = P.case_cfg(tag)
    terms = {k: float(g.raw('%s_%s' % (k, tag))) for k in R.SCALARS}
    if cfg.penalty_smooth != 'charbonnier' or cfg.closed_form_smooth:
        assert terms['smooth'] > 0.05 * abs(terms['total']), (tag, terms)  # the smoothness term carries weight (edge_asymp 0.5)
    if cfg.w_occ > 0:
        assert float(restated[tag]['occ']) > 0


@pytest.mark.parametrize('mutation', list(P.MUTATIONS))
def test_mutations_leave_the_bounds(golden, mutation):
    g = golden('elbo_penalty')
    tag = P.MUTATIONS[mutation]
    worst = _worst_ratio(g, tag, P.loss(P.case_cfg(tag), _case(g, tag), mutate=mutation))
    print(mutation, tag, 'largest error / bound %.3g' % max(worst.values()))
    assert max(worst.values()) > 100.0, (mutation, worst)


# ---- the penalty pairs --------------------------------------------------------------------------------------------------
def _args(kind):
    x = torch.cat([torch.zeros(1, dtype=P.D), torch.logspace(-6, 2.5, 200, dtype=P.D)])
    if kind in (P.GMM, P.GMM_SQ):
        pi, beta = (P.CENSUS_PI, P.CENSUS_BETA) if kind == P.GMM else (P.SMOOTH_PI, P.SMOOTH_BETA)
        return x, P.mixture(pi, beta)
    return x, None


@pytest.mark.parametrize('kind', range(5))
def test_derivative_is_the_derivative(kind):
    x, mix = _args(kind)
    x = x[1:].clone().requires_grad_(True)
    r, d = P.rho(kind, x, mix)
    auto, = torch.autograd.grad(r.sum(), x)
    assert torch.allclose(auto, d.detach(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('kind', range(5))
def test_fp32_evaluation_sits_inside_the_bounds(kind):
    """plain fp32 torch arithmetic in the kernel's order, on fp32 arguments: inside rho_bound(dx = 0) with 2x room"""
    x, mix = _args(kind)
    x = x.float()
    r64, d64 = P.rho(kind, x.double(), mix)
    rb, db = P.rho_bound(kind, x.double(), 0.0, mix)
    if kind == P.IDENTITY:
        r32, d32 = x, torch.ones_like(x)
    elif kind == P.CHARBONNIER:
        r32 = torch.sqrt(x + 1e-6)
        d32 = 0.5 / r32
    elif kind == P.ABS_ROBUST:
        lg = torch.log2(x.abs() + 0.01)
        r32, d32 = torch.exp2(0.4 * lg), 0.4 * torch.exp2(-0.6 * lg)
    else:
        w, beta = (t.float() for t in mix)
        q = x if kind == P.GMM_SQ else x * x
        arg = (-beta * q.unsqueeze(-1)) / 2
        c = arg.max(-1).values
        t = w * torch.exp(arg - c.unsqueeze(-1))
        den, num = t.sum(-1), (t * beta).sum(-1)
        r32 = -(c + torch.log(den))
        d32 = (num / den) / 2 if kind == P.GMM_SQ else (num / den) * x
    er, ed = (r32.double() - r64).abs(), (d32.double() - d64).abs()
    print(kind, 'rho: largest err / bound %.3f, rho\': %.3f' % (float((er / rb.clamp_min(1e-300)).max()),
                                                                 float((ed / db.clamp_min(1e-300)).max()) if kind else 0.0))
    assert (er <= 0.5 * rb).all() and (ed <= 0.5 * db).all()


def test_mixture_at_zero_and_weights():
    w, beta = P.mixture(P.CENSUS_PI, P.CENSUS_BETA, fp32=False)
    r, d = P.rho(P.GMM, torch.zeros(1, dtype=P.D), (w, beta))
    assert abs(float(r) + math.log(float(w.sum()))) < 1e-15 and float(d) == 0.0
    r, d = P.rho(P.GMM_SQ, torch.zeros(1, dtype=P.D), (w, beta))
    assert float(d) == pytest.approx(float((w * beta).sum() / w.sum()) / 2, rel=1e-14)  # finite at x_sq = 0
    assert float(w[0]) == pytest.approx(P.CENSUS_PI[0] * math.sqrt(P.CENSUS_BETA[0]) / math.sqrt(2 * math.pi), rel=1e-15)


def test_penalty_functions_mirror_the_reference():
    from arflow_amd.losses import penalty_functions as F
    x = torch.linspace(0, 9, 19, dtype=torch.float64)
    assert torch.equal(F.get_penalty('identity')(x), x) and torch.equal(F.get_penalty('identity', True)(x), torch.ones_like(x))
    assert torch.allclose(F.get_penalty('charbonnier')(x), torch.sqrt(x + 1e-6))
    assert torch.allclose(F.get_penalty('charbonnier', True)(x), 0.5 / torch.sqrt(x + 1e-6))
    assert torch.allclose(F.get_penalty('abs_robust_loss')(x), (x.abs() + 0.01) ** 0.4)
    with pytest.raises(NotImplementedError):
        F.get_penalty('abs_robust_loss', True)
    with pytest.raises(NotImplementedError):
        F.get_penalty('l1')
    # the squared mixture form: one node, plain torch, finite gradient at 0, equal to the restatement
    f = F.get_penalty('gmm', pi=P.SMOOTH_PI, beta=P.SMOOTH_BETA, squared=True)
    xs = torch.cat([torch.zeros(1, dtype=torch.float64), x]).requires_grad_(True)
    y = f(xs)
    gx, = torch.autograd.grad(y.sum(), xs)
    r, d = P.rho(P.GMM_SQ, xs.detach(), P.mixture(P.SMOOTH_PI, P.SMOOTH_BETA, fp32=False))
    assert torch.allclose(y.detach(), r, rtol=1e-13) and torch.allclose(gx, d, rtol=1e-13) and bool(torch.isfinite(gx).all())
    for bad in (dict(pi=None, beta=[1.0]), dict(pi=[1.0], beta=[1.0, 2.0]), dict(pi=[1.0 / 17] * 17, beta=[1.0] * 17),
                dict(pi=[1.0], beta=[0.0]), dict(pi=[-0.1], beta=[1.0]), dict(pi=[1.0], beta=[float('nan')]),
                dict(pi=[1.0, 0.0], beta=[2.0, 1.0])):  # no weight on the widest component
        with pytest.raises(ValueError):
            F.get_penalty('gmm', **bad)


# ---- the loss's settings ------------------------------------------------------------------------------------------------
def _loss(**change):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    return get_loss(AttrDict(dict(P.case_cfg('gmm_all_mean_sparse'), **change)))


def test_every_case_builds_and_the_default_flag():
    from arflow_amd import _lib
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss, UFlowElboPenLoss
    for tag in P.CASES:  # get_loss hands every non-default setting to the subclass; the base class refuses it, as it always has
        loss = get_loss(AttrDict(P.case_cfg(tag)))
        assert type(loss) is UFlowElboPenLoss and not loss.default, tag
        with pytest.raises(NotImplementedError):
            UFlowElboLoss(AttrDict(P.case_cfg(tag)))
    loss = _loss()
    assert (loss.data_pen.kind, loss.data_pen.k, loss.smooth_pen.kind, loss.smooth_pen.k) == (_lib.PEN_GMM, 10, _lib.PEN_GMM_SQ, 10)
    w, beta = P.mixture(P.CENSUS_PI, P.CENSUS_BETA)
    assert [loss.data_pen.w[j] for j in range(10)] == w.tolist() and [loss.data_pen.beta[j] for j in range(10)] == beta.tolist()
    for tag in R.CASES:  # every existing configuration keeps the calls it has
        loss = get_loss(AttrDict(R.case_cfg(tag)))
        assert type(loss) is UFlowElboLoss and loss.default, tag
    assert UFlowElboPenLoss(AttrDict(R.case_cfg('diag'))).default  # the default triple through the subclass: the base's calls
    assert get_loss(AttrDict(dict(R.case_cfg('diag'), penalty_smooth='identity'))).smooth_pen.kind == _lib.PEN_IDENTITY


@pytest.mark.parametrize('change', [
    dict(penalty_census_pi=None), dict(penalty_smooth_beta=None), dict(penalty_census_pi=P.CENSUS_PI[:9]),
    dict(penalty_smooth_pi=[1.0 / 17] * 17, penalty_smooth_beta=[1.0] * 17), dict(penalty_census_beta=[0.0] + P.CENSUS_BETA[1:]),
    dict(penalty_smooth_beta=[-1.0] + P.SMOOTH_BETA[1:]), dict(penalty_census_pi=[-0.1] + P.CENSUS_PI[1:])])
def test_malformed_mixtures_raise_value_error(change):
    with pytest.raises(ValueError):
        _loss(**change)


def test_a_missing_key_is_a_value_error():
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    cfg = dict(R.case_cfg('diag'), penalty_smooth='gmm')  # no penalty_smooth_pi / _beta at all
    with pytest.raises(ValueError, match='penalty_smooth_pi'):
        get_loss(AttrDict(cfg))


@pytest.mark.parametrize('change,match', [
    (dict(occ_type='none'), "occ_type: 'none'"), (dict(data_loss=['ssim']), r"data_loss: \['ssim'\]"),
    (dict(data_penalty=['gmm', 'gmm']), 'data_penalty'), (dict(data_penalty=['l1']), r"data_penalty: \['l1'\]"),
    (dict(penalty_smooth='l1'), "penalty_smooth: 'l1'"), (dict(isotropic_smooth=True), 'isotropic_smooth: True'),
    (dict(approx='mixture', n_components=2), "occ_type: 'mean' with approx: 'mixture'")])
def test_settings_that_still_raise(change, match):
    with pytest.raises(NotImplementedError, match=match):
        _loss(**change)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import os
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _pen(kind, k=0, w=None, beta=None):
    from arflow_amd import _lib
    d = _lib.Penalty()
    d.kind, d.k = kind, k
    for j in range(k if 0 <= k <= 16 else 0):
        d.w[j] = 0.1 if w is None else w[j]
        d.beta[j] = 1.0 if beta is None else beta[j]
    return d


def test_argument_errors_of_the_penalised_entry_points(lib):
    """Every call here is REJECTED by the argument checks, which run before any launch: the pointers are never dereferenced,
    with or without a GPU in the machine.  A descriptor one family accepts is therefore only ever handed to the other family."""
    from arflow_amd import _lib
    one = ctypes.c_void_p(16)
    H = W = 8

    def census(pen):
        p = None if pen is None else ctypes.addressof(pen)
        return {lib.arflow_census_warp_pen_fwd(one, one, one, 2 * H * W, None, None, one, one, 2, H, W, 3, None, 0, p, None),
                lib.arflow_census_warp_pair_pen_fwd(one, one, 2 * H * W, None, None, one, one, 2, H, W, 3, None, 0, p, None),
                lib.arflow_census_pen_fwd(one, one, one, one, one, one, 2, H, W, 3, p, None)}

    def smooth(pen):
        p = None if pen is None else ctypes.addressof(pen)
        return {lib.arflow_smooth_pen_fwd(one, one, one, 2, 3, H, W, 2 * H * W, 1.0, 10.0, 1, 1, p, None),
                lib.arflow_smooth_pen_bwd(one, one, one, one, 2, 3, H, W, 2 * H * W, 1.0, 10.0, 1, 1, p, None)}
    assert census(None) == {-1001} and smooth(None) == {-1001}                          # NULL descriptor
    for bad in (_pen(-1), _pen(5), _pen(_lib.PEN_GMM, 0), _pen(_lib.PEN_GMM, 17), _pen(_lib.PEN_GMM_SQ, 0), _pen(_lib.PEN_GMM_SQ, 17)):
        assert census(bad) == {-1003} and smooth(bad) == {-1003}, (bad.kind, bad.k)     # unknown kind, k outside 1..16
    assert census(_pen(_lib.PEN_GMM_SQ, 2)) == {-1003}                                  # GMM_SQ in a census call
    assert smooth(_pen(_lib.PEN_GMM, 2)) == {-1003}                                     # GMM in a smoothness call
    for kw in (dict(beta=[1.0, 0.0]), dict(beta=[1.0, -2.0]), dict(beta=[float('inf'), 1.0]), dict(beta=[1.0, float('nan')]),
               dict(w=[0.1, -0.1]), dict(w=[float('nan'), 0.1]),
               dict(w=[0.1, 0.0], beta=[2.0, 1.0])):  # no weight on the widest component: the density can underflow to 0
        assert census(_pen(_lib.PEN_GMM, 2, **kw)) == {-1003}, kw
        assert smooth(_pen(_lib.PEN_GMM_SQ, 2, **kw)) == {-1003}, kw
    # the other arguments keep the contract of the unpenalised entry points
    ok = _pen(_lib.PEN_IDENTITY)
    p = ctypes.addressof(ok)
    assert lib.arflow_census_warp_pen_fwd(None, one, one, 2 * H * W, None, None, one, one, 2, H, W, 3, None, 0, p, None) == -1001
    assert lib.arflow_census_warp_pen_fwd(one, one, one, 2 * H * W, None, None, one, one, 2, H, 10, 3, None, 0, p, None) == -1002
    assert lib.arflow_census_warp_pen_fwd(one, one, one, 2 * H * W, None, None, one, one, 2, H, W, 3, one, 2 * H * W - 1, p, None) == -1002
    assert lib.arflow_census_warp_pen_fwd(one, one, one, 2 * H * W, None, None, one, one, 2, H, W, 4, None, 0, p, None) == -1003
    assert lib.arflow_census_warp_pair_pen_fwd(one, one, 2 * H * W, None, None, one, one, 3, H, W, 3, None, 0, p, None) == -1002
    assert lib.arflow_census_pen_fwd(one, one, None, one, one, one, 2, H, W, 3, p, None) == -1001      # the mask is required
    assert lib.arflow_census_pen_fwd(one, one, one, None, one, one, 2, H, W, 3, p, None) == -1001      # and so is ham
    for radius in (0, 4, 16):
        assert lib.arflow_census_pen_fwd(one, one, one, one, one, one, 2, H, W, radius, p, None) == -1003
    assert lib.arflow_smooth_pen_fwd(one, one, one, 2, 3, H, W, 2 * H * W, 1.0, 10.0, 3, 1, p, None) == -1003
    assert lib.arflow_smooth_pen_bwd(one, one, None, one, 2, 3, H, W, 2 * H * W, 1.0, 10.0, 1, 1, p, None) == -1001


def test_descriptor_layout_matches_the_header():
    from arflow_amd import _lib
    assert ctypes.sizeof(_lib.Penalty) == 8 + 2 * 4 * 16 and _lib.Penalty.w.offset == 8 and _lib.Penalty.beta.offset == 72
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'arflow_hip.h')).read()
    for i, name in enumerate(('IDENTITY', 'CHARBONNIER', 'ABS_ROBUST', 'GMM', 'GMM_SQ')):
        assert '#define ARFLOW_PEN_%s %d\n' % (name, i) in text and getattr(_lib, 'PEN_' + name) == i


def test_penalty_cfg_round_trip():
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    from arflow_amd.penalty_em import penalty_cfg
    fit = penalty_cfg(torch.tensor(P.CENSUS_PI, dtype=torch.float64), torch.tensor(P.CENSUS_BETA, dtype=torch.float64), scale=2.5)
    assert fit['pi'] == P.CENSUS_PI and fit['beta'] == [2.5 * b for b in P.CENSUS_BETA]
    assert all(type(v) is float for v in fit['pi'] + fit['beta'])
    cfg = dict(R.case_cfg('diag'), data_penalty=['gmm'], penalty_census_pi=fit['pi'], penalty_census_beta=fit['beta'])
    loss = get_loss(AttrDict(cfg))
    assert loss.data_pen.k == 10 and loss.data_pen.beta[0] == np.float32(2.5 * P.CENSUS_BETA[0])
    with pytest.raises(ValueError):
        penalty_cfg([0.5, 0.5], [1.0])
