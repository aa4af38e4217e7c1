"""CPU: the float64 restatement of the mixture family (tests/mixture_ref.py) against what the reference's own code computed
(tests/golden/elbo_mixture.npz), its closed-form gradients against central differences, plus everything of the new operators,
loss, model and workload that does not need a GPU: the raw entry points' error codes, the argument checks, the unsupported
settings, ComponentNet's keys."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mixture_ref as R


def _rel(got, ref):
    scale = max(np.abs(ref).max(), 1e-300)
    return np.abs(got - ref).max() / scale


def _loss_case(g, tag):
    names = ['net12', 'net21', 'eps12', 'eps21', 'comp12', 'comp21'] + (['weights12', 'weights21'] if tag in R.WEIGHTED else [])
    case = {k: g.raw('%s_%s' % (k, tag)) for k in names}
    case.update(im1=g.raw('im1'), im2=g.raw('im2'))
    return case


@pytest.mark.parametrize('tag', list(R.CASES))
def test_loss_restatement_matches_the_reference(golden, tag):
    g = golden('elbo_mixture')
    case = _loss_case(g, tag)
    recipe = R.make_loss_case(tag)
    assert sorted(case) == sorted(recipe) and all(np.array_equal(case[k], recipe[k]) for k in case)
    cfg = R.case_cfg(tag)
    got = R.loss(cfg, case)
    for key in R.case_outputs(tag):
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        print('%s %s: rel %.3e' % (tag, key, _rel(got[key], ref)))
        assert _rel(got[key], ref) <= 1e-10, key
    total = got['warp'] + got['smooth'] - got['entropy'] + got['oof'] + got['occ']
    assert abs(total - got['total']) <= 1e-13 * abs(total)
    # the operator restatements are what the loss restatement is made of
    K, S, B = cfg.n_components, cfg.n_samples, R.LOSS_B
    entropy = 0.
    for d in (('12', '21') if cfg.with_bk else ('12',)):
        net = case['net' + d]
        w = case['weights' + d] if tag in R.WEIGHTED else np.full((B, K), 1.0 / K)
        den = R.density(net[:, :2 * K], net[:, 2 * K:], w, case['comp' + d], case['eps' + d], S)
        if d == '12':
            assert _rel(den['flow'], g.raw('flow12_2_' + tag)) <= 1e-12
        entropy -= cfg.w_entropy * den['logpdf'].mean()
    assert abs(entropy - got['entropy']) <= 1e-12 * abs(got['entropy'])
    # the draws are mixed within an item, and the tie case's responsibilities are not one-hot
    assert all(len(set(row)) > 1 for row in case['comp12'].tolist())
    if tag == 'mix2_tie':
        assert float(g.raw('resp_min_' + tag)) >= 0.05


def test_closed_form_weight_gradients_match_the_reference(golden):
    """gweights of mix3w from the closed form sum_s glogpdf[n] q[n,k] / P with glogpdf = -w_entropy / (S B)."""
    g = golden('elbo_mixture')
    tag = 'mix3w'
    case, cfg = _loss_case(g, tag), R.case_cfg(tag)
    K, S, B = cfg.n_components, cfg.n_samples, R.LOSS_B
    for d in ('12', '21'):
        net = case['net' + d]
        glp = np.full(S * B, cfg.w_entropy / (S * B))  # total = ... - loss_entropy, loss_entropy = -w mean(logpdf)
        res = R.grads(net[:, :2 * K], net[:, 2 * K:], case['weights' + d], case['comp' + d], case['eps' + d], None, glp, S)
        assert _rel(res['gweights'], g.raw('gweights%s_%s' % (d, tag))) <= 1e-10


def test_entropy_map_restatement_matches_the_reference(golden):
    g = golden('elbo_mixture')
    case = {k: g.raw(k + '_entropy_map') for k in ('mean', 'log_std', 'weights', 'comp', 'eps')}
    recipe = R.make_entropy_case()
    assert all(np.array_equal(case[k], recipe[k]) for k in case)
    got, mag = R.entropy_map(case['mean'], case['log_std'], case['weights'], case['comp'], case['eps'], R.ENTROPY_N)
    ref = g.raw('out_entropy_map')
    assert got.shape == ref.shape == (2, 1, 8, 16) and ref.dtype == np.float64
    assert _rel(got, ref) <= 1e-10 and (mag > 0).all()


@pytest.mark.parametrize('K,comp,weights', [(1, 'equal', 'uniform'), (2, 'mixed', 'uniform'), (3, 'mixed', 'nonuniform'),
                                            (4, 'equal', 'zero')])
def test_gradients_against_central_differences(K, comp, weights):
    """The closed-form gradients of mixture_ref.grads against central differences of mixture_ref.objective on a 3 x 5 level,
    along random directions in mean, log_std and the weights."""
    B, S, M, N = 2, 3, 3, 5
    c = R.make_case(B, S, K, M, N, comp=comp, weights=weights)
    args = lambda mean, ls, w: (mean, ls, w, c['comp'], c['eps'], c['gZ'], c['glogpdf'], S)  # noqa: E731
    mean, ls, w = (c[k].astype(np.float64) for k in ('mean', 'log_std', 'weights'))
    res = R.grads(*args(mean, ls, w)[:5], c['gZ'], c['glogpdf'], S)
    r = res['den']['resp']
    if K > 1 and weights != 'zero':
        assert float(np.minimum(r, 1 - r).max()) > 0.05  # the cross-component terms are exercised
    if weights == 'zero':
        assert (r[:, K - 1] == 0).all() and np.isfinite(res['den']['q']).all()
    rng = np.random.default_rng(9)
    h = 1e-6
    for name, grad, x in (('gmean', res['gmean'], mean), ('glog_std', res['glog_std'], ls), ('gweights', res['gweights'], w)):
        dirn = rng.standard_normal(x.shape)
        if name == 'gweights':
            dirn = dirn * (w > 0)  # a zero weight stays zero (its one-sided derivative is q / P, checked above)
        i = ('gmean', 'glog_std', 'gweights').index(name)
        plus = tuple(v + h * dirn if j == i else v for j, v in enumerate((mean, ls, w)))
        minus = tuple(v - h * dirn if j == i else v for j, v in enumerate((mean, ls, w)))
        num = (R.objective(*args(*plus)) - R.objective(*args(*minus))) / (2 * h)
        assert abs(num - (grad * dirn).sum()) <= 1e-6 * np.abs(grad * dirn).sum() + 1e-9, name
    if K == 1:  # the two routes through logpdf cancel in the mean
        fold = sum(c['gZ'][s * B:(s + 1) * B].astype(np.float64) for s in range(S))
        assert np.allclose(res['gmean'], fold, rtol=0, atol=1e-12)


def test_raw_entry_points_check_their_arguments():
    from arflow_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ok = dict(B=2, S=2, K=3, M=4, N=5)  # items: 2 K M N = 120 floats, samples: 2 M N = 40

    def sample(mean=one, ls=one, eps=one, comp=one, flow=one, work=one, mbs=120, lbs=120, ebs=40, fbs=40, **kw):
        a = dict(ok, **kw)
        return lib.arflow_mixture_sample_fwd(mean, mbs, ls, lbs, eps, ebs, comp, flow, fbs, work, a['B'], a['S'], a['K'], a['M'],
                                             a['N'], None)

    def logpdf(work=one, weights=one, lp=one, resp=one, q=one, **kw):
        a = dict(ok, **kw)
        return lib.arflow_mixture_logpdf_fwd(work, weights, lp, resp, q, a['B'], a['S'], a['K'], a['M'], a['N'], None)

    def bwd(mean=one, ls=one, eps=one, comp=one, resp=one, glp=one, gZ=one, gmean=one, gls=one, mbs=120, lbs=120, ebs=40,
            gzbs=40, gmbs=120, glbs=120, **kw):
        a = dict(ok, **kw)
        return lib.arflow_mixture_bwd(mean, mbs, ls, lbs, eps, ebs, comp, resp, glp, gZ, gzbs, gmean, gmbs, gls, glbs, a['B'],
                                      a['S'], a['K'], a['M'], a['N'], None)

    def entropy(mean=one, ls=one, weights=one, comp=one, eps=one, out=one, mbs=120, lbs=120, ebs=40, **kw):
        a = dict(ok, **kw)
        return lib.arflow_mixture_entropy_map(mean, mbs, ls, lbs, weights, comp, eps, ebs, out, a['B'], a['S'], a['K'], a['M'],
                                              a['N'], None)

    for fn, ptrs in ((sample, ('mean', 'ls', 'eps', 'comp', 'flow', 'work')), (logpdf, ('work', 'weights', 'lp', 'resp', 'q')),
                     (bwd, ('mean', 'ls', 'eps', 'comp', 'gmean', 'gls')), (entropy, ('mean', 'ls', 'weights', 'comp', 'eps', 'out'))):
        for name in ptrs:
            assert fn(**{name: None}) == -1001, (fn.__name__, name)
        for K in (0, 5):
            assert fn(K=K) == -1003, (fn.__name__, K)
        for change in (dict(B=0), dict(S=0), dict(M=0), dict(N=0), dict(M=65536, N=32768), dict(B=256, S=256)):
            assert fn(**change) == -1002, (fn.__name__, change)
    for fn in (sample, bwd, entropy):
        for change in (dict(mbs=119), dict(lbs=119), dict(ebs=39)):
            assert fn(**change) == -1002, (fn.__name__, change)
    assert sample(fbs=39) == -1002
    assert bwd(gzbs=39) == -1002 and bwd(gmbs=119) == -1002 and bwd(glbs=119) == -1002
    assert bwd(resp=None) == -1001       # needed by the source that is present
    assert lib.arflow_mixture_work_size(2, 3, 2, 4, 5) == 3 * 2 * 1 * 2
    assert lib.arflow_mixture_work_size(1, 3, 4, 40, 52) == 3 * -(-40 * 52 // R.CHUNK) * 4
    assert lib.arflow_mixture_work_size(1, 1, 5, 4, 5) == -1003 and lib.arflow_mixture_work_size(0, 1, 2, 4, 5) == -1002
    assert lib.arflow_abi_version() == 10


def test_python_functions_refuse_cpu_tensors_and_check_arguments():
    from arflow_amd import _lib, mixture as MX
    mean, ls, w = torch.zeros(2, 4, 3, 5), torch.zeros(2, 4, 3, 5), torch.full((2, 2), 0.5)
    comp, eps = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(6, 2, 3, 5)
    with pytest.raises(_lib.ArflowHipError):
        MX.reparam_gmm(mean, ls, w, 3, comp=comp, eps=eps)
    with pytest.raises(_lib.ArflowHipError):
        MX.reparam_gmm(mean, ls, w, 3)
    with pytest.raises(_lib.ArflowHipError):
        MX.gaussian_mixture_log_pdf(None, mean, ls, w, 3, comp=comp, eps=eps)
    net = torch.cat((mean, ls), 1)
    with pytest.raises(_lib.ArflowHipError):
        MX.reparam_gmm_pair((net, w, comp, eps), (net, w, comp, eps), 3)
    with pytest.raises(_lib.ArflowHipError):
        MX.mixture_entropy(mean, ls, w, 3, comp=comp, eps=eps)
    with pytest.raises(NotImplementedError, match='flow=None'):
        MX.gaussian_mixture_log_pdf(eps, mean, ls, w, 3)
    for bad, match in ((None, 'mean'), (torch.zeros(2, 5, 3, 5), 'mean'), (torch.zeros(2, 10, 3, 5), 'mean'),
                       (torch.zeros(4, 3, 5), 'mean')):
        with pytest.raises(ValueError, match=match):
            MX.mixture_entropy(bad, ls, w, 3, comp=comp, eps=eps)
    with pytest.raises(ValueError, match='n_samples'):
        MX.mixture_entropy(mean, ls, w, 0)
    with pytest.raises(ValueError, match='net must be'):
        MX.reparam_gmm_pair((torch.zeros(2, 6, 3, 5), w, comp, eps), (net, w, comp, eps), 3)

    # the checks that follow the device check, on the checkers themselves (a stand-in that reports is_cuda)
    class Fake(torch.Tensor):
        is_cuda = True
    fake = lambda *shape, **kw: torch.zeros(*shape, **kw).as_subclass(Fake)  # noqa: E731
    assert MX._check('mean', fake(2, 11, 3, 5)[:, 1:5], (2, 4, 3, 5)) == 165   # a channel slice is a valid layout
    with pytest.raises(ValueError, match='log_std must be float32'):
        MX._check('log_std', fake(2, 4, 3, 5, dtype=torch.float64), (2, 4, 3, 5))
    with pytest.raises(ValueError, match='eps must be'):
        MX._inputs(fake(2, 4, 3, 5), fake(2, 4, 3, 5), fake(2, 3, dtype=torch.int64), fake(5, 2, 3, 5), 3)
    with pytest.raises(ValueError, match='comp must be torch.int64'):
        MX._inputs(fake(2, 4, 3, 5), fake(2, 4, 3, 5), fake(2, 3, dtype=torch.int32), fake(6, 2, 3, 5), 3)
    with pytest.raises(ValueError, match='comp must be'):
        MX._inputs(fake(2, 4, 3, 5), fake(2, 4, 3, 5), fake(3, 2, dtype=torch.int64), fake(6, 2, 3, 5), 3)
    with pytest.raises(ValueError, match='weights must be'):
        MX._small('weights', fake(2, 3), (2, 2), torch.float32, fake(1))


NONE = object()


@pytest.mark.parametrize('change,exc,match', [
    (dict(n_components=1), NotImplementedError, "approx: 'mixture' with n_components: 1"),
    (dict(n_components=5), NotImplementedError, "approx: 'mixture' with n_components: 5"),
    (dict(n_components=2.5), NotImplementedError, "approx: 'mixture' with n_components: 2.5"),
    (dict(n_components=NONE), NotImplementedError, "approx: 'mixture' with n_components: None"),
    (dict(closed_form_smooth=True), NotImplementedError, 'closed_form_smooth'),
])
def test_unsupported_settings_raise_at_construction(change, exc, match):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    cfg = dict(R.case_cfg('mix2'), **change)
    cfg = {k: v for k, v in cfg.items() if v is not NONE}
    with pytest.raises(exc, match=match):
        get_loss(AttrDict(cfg))


def test_loss_constructs_checks_channels_and_has_no_cpu_path():
    from arflow_amd import _lib
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    for tag in R.CASES:
        assert isinstance(get_loss(AttrDict(R.case_cfg(tag))), UFlowElboLoss)
    for K in (2, 3, 4):
        get_loss(AttrDict(dict(R.case_cfg('mix2'), n_components=K)))
    loss = get_loss(AttrDict(R.case_cfg('mix3w')))
    im = torch.zeros(1, 3, 8, 8)
    for C in (8, 13):
        net = torch.zeros(1, C, 2, 2)
        with pytest.raises(ValueError, match='n_components 3 needs 12 level-2 channels \\(got %d\\)' % C):
            loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)
    net = torch.zeros(1, 12, 2, 2)
    with pytest.raises(_lib.ArflowHipError):
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)
    # inv_cov: the reference's sentence, in forward, before anything touches the GPU
    loss = get_loss(AttrDict(dict(R.case_cfg('mix2'), inv_cov=True)))
    with pytest.raises(NotImplementedError, match='Inverse covariance parametrization is not implemented for mixture '
                                                  'variational approximation.'):
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)
    # component draws belong to the mixture only
    loss = get_loss(AttrDict(dict(R.case_cfg('mix2'), approx='diag')))
    with pytest.raises(ValueError, match='comp'):
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im, comp=(None, None))


def test_get_loss_dispatches_on_type_only():
    import inspect
    from arflow_amd.losses.get_loss import get_loss
    assert 'approx' not in inspect.getsource(get_loss)


def test_component_net_keys_parameters_and_refusals(golden):
    from arflow_amd.models import get_model
    from arflow_amd.models.uflow_prob_model import ComponentNet, PWCProbFlow
    from tests import prob_ref as P
    g = golden('elbo_mixture')
    model = get_model(R.model_cfg())
    assert isinstance(model, ComponentNet)
    assert isinstance(model.pwcnet1, PWCProbFlow) and isinstance(model.pwcnet2, PWCProbFlow)
    keys = list(model.state_dict().keys())
    assert sorted(keys) == g['keys_component']
    assert all(k.startswith(('pwcnet1.', 'pwcnet2.')) for k in keys)
    assert keys[:len(keys) // 2] == ['pwcnet1.' + k.split('.', 1)[1] for k in keys[len(keys) // 2:]]  # pwcnet1 first
    n = sum(p.numel() for p in model.parameters())
    assert n == 2 * P.PARAMS[(2, 2, 0)] == int(g.raw('params_component'))
    for sub in (model.pwcnet1, model.pwcnet2):
        assert list(sub.cfg.out_channels) == [2, 2, 0] and sub.cfg.n_pyramids == 1 and not sub.cfg.mixture_weights
    assert model.cfg.n_pyramids == 2  # the caller's cfg is not modified
    with pytest.raises(NotImplementedError, match='mixture_weights = True'):
        get_model(type(R.model_cfg())(dict(R.model_cfg(), mixture_weights=True)))
    model.init_weights()
    assert all(float(p.abs().max()) == 0 for k, p in model.named_parameters() if k.endswith('bias'))


def test_workload_entry_builds_model_and_loss():
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    from arflow_amd.models import get_model
    from arflow_amd.models.uflow_prob_model import ComponentNet
    from arflow_amd.train_step import WORKLOADS
    mcfg, lcfg = WORKLOADS['componentnet+uflow_elbo_mixture']
    assert mcfg['type'] == 'component' and mcfg['out_channels'] == [2, 2, 0] and mcfg['level_dropout'] == 0.1
    assert mcfg['feature_norm'] and not mcfg['inv_cov'] and not mcfg['mixture_weights']
    assert lcfg['approx'] == 'mixture' and lcfg['n_components'] == 2 and lcfg['n_samples'] == 6 and lcfg['w_entropy'] == 0.3
    assert lcfg['with_bk'] and not lcfg['inv_cov'] and lcfg['edge_asymp'] == 0.01 and lcfg['edge_constant'] == 150
    assert lcfg['w_oof'] == 0.0 and lcfg['w_occ'] == 0.0 and lcfg['closed_form_smooth'] is False
    assert isinstance(get_model(AttrDict(mcfg)), ComponentNet)
    assert get_loss(AttrDict(lcfg)).cfg.approx == 'mixture'
