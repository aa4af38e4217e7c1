"""CPU: the float64 restatement of the low-rank family (tests/lowrank_ref.py) against what the reference's own code computed
(tests/golden/elbo_lowrank.npz), plus everything of the new operators, loss, model and workload that does not need a GPU: the
adjoint identity, the raw entry points' error codes, the argument checks, the unsupported settings, the model's keys."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lowrank_ref as R


def _rel(got, ref):
    scale = max(np.abs(ref).max(), 1e-300)
    return np.abs(got - ref).max() / scale


def _loss_case(g, tag):
    case = {k: g.raw('%s_%s' % (k, tag)) for k in ('net12', 'net21', 'eps12', 'eps21')}
    case.update(im1=g.raw('im1'), im2=g.raw('im2'))
    return case


@pytest.mark.parametrize('tag', list(R.CASES))
def test_loss_restatement_matches_the_reference(golden, tag):
    g = golden('elbo_lowrank')
    case = _loss_case(g, tag)
    recipe = R.make_loss_case(tag)
    assert all(np.array_equal(case[k], recipe[k]) for k in case)
    cfg = R.case_cfg(tag)
    got = R.loss(cfg, case)
    for key in R.OUTPUTS:
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        print('%s %s: rel %.3e' % (tag, key, _rel(got[key], ref)))
        assert _rel(got[key], ref) <= 1e-12, key
    total = got['warp'] + got['smooth'] - got['entropy'] + got['oof'] + got['occ']
    assert abs(total - got['total']) <= 1e-13 * abs(total)
    # the operator restatements are what the loss restatement is made of
    S, B, Rk = cfg.n_samples, R.LOSS_B, cfg.columns
    z, _ = R.sampler(case['net12'][:, 0:2], case['net12'][:, 2:], case['eps12'], S)
    assert _rel(z, g.raw('flow12_2_' + tag)) <= 1e-12
    ld = sum(R.logdet(case[n][:, 2:])[0].sum(1).mean() for n in (('net12', 'net21') if cfg.with_bk else ('net12',)))
    assert abs(cfg.w_entropy * ld / (2 * 8 * 16) - got['entropy']) <= 1e-12 * abs(got['entropy'])
    assert case['eps12'].shape == (S * B, 2 * Rk, 1, 1)


@pytest.mark.parametrize('R_', [1, 3, 16])
def test_adjoint_identity_and_gradients(R_):
    """<z - mean, gZ> = <std, gstd> (the sampler is linear in std), gmean folds the samples, and the log-det gradient
    2 G^-1 U against a central difference of the restated log-det."""
    B, S, M, N = 2, 3, 5, 7
    c = R.make_case(B, S, R_, M, N)
    z, mag = R.sampler(c['mean'], c['std'], c['eps'], S)
    gmean, gstd, _, _ = R.grads(c['std'], c['eps'], c['gZ'], None, S)
    lhs = ((z - np.tile(c['mean'].astype(np.float64), (S, 1, 1, 1))) * c['gZ']).sum()
    rhs = (c['std'].astype(np.float64) * gstd).sum()
    assert abs(lhs - rhs) <= 1e-12 * (mag * np.abs(c['gZ'])).sum()
    assert np.allclose(gmean, sum(c['gZ'][s * B:(s + 1) * B].astype(np.float64) for s in range(S)), rtol=0, atol=1e-13)
    _, gl, _, _ = R.grads(c['std'], None, None, c['glogdet'], S)
    rng = np.random.default_rng(5)
    d = rng.standard_normal(c['std'].shape)
    h = 1e-6
    f = lambda s: (R.logdet(s)[0] * c['glogdet']).sum()  # noqa: E731
    num = (f(c['std'].astype(np.float64) + h * d) - f(c['std'].astype(np.float64) - h * d)) / (2 * h)
    assert abs(num - (gl * d).sum()) <= 1e-6 * np.abs(gl * d).sum()


def test_raw_entry_points_check_their_arguments():
    from arflow_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ok = dict(B=2, S=2, R=3, M=4, N=5)

    def sample(mean=one, std=one, eps=one, Z=one, mbs=40, sbs=120, zbs=40, **kw):
        a = dict(ok, **kw)
        return lib.arflow_lowrank_sample_fwd(mean, mbs, std, sbs, eps, Z, zbs, a['B'], a['S'], a['R'], a['M'], a['N'], None)

    def logdet(std=one, work=one, ld=one, ginv=one, sbs=120, **kw):
        a = dict(ok, **kw)
        return lib.arflow_lowrank_logdet_fwd(std, sbs, work, ld, ginv, a['B'], a['R'], a['M'], a['N'], None)

    def bwd(std=one, eps=one, gZ=one, ginv=one, gl=one, gmean=one, gstd=one, sbs=120, gzbs=40, gmbs=40, gsbs=120, **kw):
        a = dict(ok, **kw)
        return lib.arflow_lowrank_bwd(std, sbs, eps, gZ, gzbs, ginv, gl, gmean, gmbs, gstd, gsbs, a['B'], a['S'], a['R'], a['M'],
                                      a['N'], None)

    for fn, ptrs in ((sample, ('mean', 'std', 'eps', 'Z')), (logdet, ('std', 'work', 'ld', 'ginv')), (bwd, ('std', 'gstd'))):
        for name in ptrs:
            assert fn(**{name: None}) == -1001, (fn.__name__, name)
        for R_ in (0, 17):
            assert fn(R=R_) == -1003, (fn.__name__, R_)
        for change in (dict(B=0), dict(M=0), dict(N=0), dict(sbs=119), dict(M=65536, N=32768, sbs=1 << 40)):
            assert fn(**change) == -1002, (fn.__name__, change)
    assert sample(S=0) == -1002 and sample(mbs=39) == -1002 and sample(zbs=39) == -1002
    assert bwd(S=0) == -1002 and bwd(gzbs=39) == -1002 and bwd(gmbs=39) == -1002 and bwd(gsbs=119) == -1002
    assert bwd(eps=None) == -1001 and bwd(ginv=None) == -1001  # needed by the source that is present
    assert lib.arflow_lowrank_work_size(2, 3, 4, 5) == 2 * 2 * 1 * 9
    assert lib.arflow_lowrank_work_size(1, 16, 33, 65) == 2 * -(-33 * 65 // R.CHUNK) * 256
    assert lib.arflow_lowrank_work_size(1, 17, 4, 5) == -1003 and lib.arflow_lowrank_work_size(0, 3, 4, 5) == -1002
    assert lib.arflow_abi_version() == 10


def test_python_argument_checks():
    from arflow_amd import _lib, lowrank as LR
    mean, std = torch.zeros(2, 2, 4, 5), torch.zeros(2, 6, 4, 5)
    with pytest.raises(_lib.ArflowHipError):
        LR.reparam_lowrank(mean, std, 1)
    with pytest.raises(_lib.ArflowHipError):
        LR.gram_logdet(std)
    with pytest.raises(_lib.ArflowHipError):
        LR.reparam_lowrank_pair((mean, std, torch.zeros(2, 6, 1, 1)), (mean, std, torch.zeros(2, 6, 1, 1)), 1)
    for bad, match in ((None, 'std'), (torch.zeros(2, 5, 4, 5), 'std'), (torch.zeros(2, 34, 4, 5), 'std'),
                       (torch.zeros(6, 4, 5), 'std')):
        with pytest.raises(ValueError, match=match):
            LR.gram_logdet(bad)
    # the checks that follow the device check, on the checker itself (a meta tensor reports is_cuda False: use the function)
    class Fake(torch.Tensor):
        is_cuda = True
    fake = lambda *shape, **kw: torch.zeros(*shape, **kw).as_subclass(Fake)  # noqa: E731
    assert LR._check('std', fake(2, 6, 4, 5), (2, 6, 4, 5)) == 120
    assert LR._check('mean', fake(2, 8, 4, 5)[:, 0:2], (2, 2, 4, 5)) == 160      # a channel slice is a valid layout
    assert LR._check('std', fake(2, 8, 4, 5)[:, 2:], (2, 6, 4, 5)) == 160
    with pytest.raises(ValueError, match='std must be float32'):
        LR._check('std', fake(2, 6, 4, 5, dtype=torch.float64), (2, 6, 4, 5))
    with pytest.raises(ValueError, match='mean must be'):
        LR._check('mean', fake(2, 2, 4, 6), (2, 2, 4, 5))
    with pytest.raises(ValueError, match='std must be contiguous or a channel slice'):
        LR._check('std', fake(2, 6, 4, 10)[..., ::2], (2, 6, 4, 5))
    with pytest.raises(ValueError, match='eps must be'):
        LR._eps_check(fake(4, 6, 1, 1), 3, 2, 3, fake(2, 6, 4, 5))
    with pytest.raises(ValueError, match='cannot carry 3 independent columns'):
        LR._logdet_fwd(fake(2, 6, 1, 2))


NONE = object()


@pytest.mark.parametrize('change,exc,match', [
    (dict(columns=NONE), NotImplementedError, "approx: 'lowrank' needs `columns`"),
    (dict(columns=0), NotImplementedError, 'columns: 0'),
    (dict(columns=17), NotImplementedError, 'columns: 17'),
    (dict(closed_form_smooth=True), NotImplementedError, 'closed_form_smooth'),
    (dict(inv_cov=True), NotImplementedError, 'inv_cov: True'),
])
def test_unsupported_settings_raise_at_construction(change, exc, match):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    cfg = dict(R.case_cfg('lr3'), **change)
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
    loss = get_loss(AttrDict(R.case_cfg('lr3')))
    im = torch.zeros(1, 3, 8, 8)
    for C in (7, 10):
        net = torch.zeros(1, C, 2, 2)
        with pytest.raises(ValueError, match='columns 3 needs 8 level-2 channels'):
            loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)
    net = torch.zeros(1, 8, 2, 2)
    with pytest.raises(_lib.ArflowHipError):
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)


def test_workload_entry_is_the_shipped_config():
    from arflow_amd.train_step import WORKLOADS
    mcfg, lcfg = WORKLOADS['pwcprobflow+uflow_elbo_lowrank']
    assert mcfg['type'] == 'uflow_prob' and mcfg['out_channels'] == [2, 0, 30] and mcfg['level_dropout'] == 0.0
    assert lcfg['approx'] == 'lowrank' and lcfg['columns'] == 15 and lcfg['n_samples'] == 4 and lcfg['w_entropy'] == 0.1
    assert lcfg['with_bk'] and not lcfg['inv_cov'] and lcfg['edge_asymp'] == 0.01
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    get_loss(AttrDict(lcfg))


@pytest.mark.parametrize('tag', list(R.MODEL_CASES))
def test_model_keys_parameter_count_and_outputs(golden, tag):
    from arflow_amd.models import get_model
    g = golden('elbo_lowrank')
    model = get_model(R.model_cfg(tag))
    assert list(model.state_dict().keys()) == g['keys_' + tag]
    assert sum(p.numel() for p in model.parameters()) == int(g.raw('params_' + tag))
    # the composed path on the oracle ops against the reference's outputs (gate of tests/test_prob_model_cpu.py)
    from tests import prob_ref as P
    from tests.helpers import epe, oracle_ops
    img1, img2, insum = P.make_input()
    assert insum == float(g['insum'])
    R.prepare(model)
    torch.set_num_threads(8)
    with torch.no_grad(), oracle_ops(model):
        res = model(img1, img2, with_bk=True)
    assert [f.shape[1] for f in res['flows_fw']] == [sum(R.MODEL_CASES[tag])] * 3 + [2] * 3
    for name, arr in R.collect(res, tag).items():
        ref, arr = torch.as_tensor(np.asarray(g[name])), torch.from_numpy(arr)
        assert arr.shape == ref.shape, name
        for c in range(0, arr.shape[1], 2):
            assert epe(arr[:, c:c + 2], ref[:, c:c + 2]) <= 1e-3, (name, c)


def test_entropy_map_of_the_inference_tool():
    """inference.py:76-84 restated: log(sum_k std_k^2) / 2 + 2 log 4, x4 bilinear (align_corners=False)."""
    from arflow_amd.inference import lowrank_entropy_map
    std = torch.from_numpy(R.make_case(1, 1, 3, 4, 5)['std']).double()
    got = lowrank_entropy_map(std)
    u = torch.log((std[:, 0::2] ** 2).sum(1, keepdim=True)) / 2
    v = torch.log((std[:, 1::2] ** 2).sum(1, keepdim=True)) / 2
    ref = torch.nn.functional.interpolate(torch.cat((u, v), 1) + 2 * np.log(4.0), scale_factor=4, mode='bilinear',
                                          align_corners=False)
    assert got.shape == (1, 2, 16, 20) and torch.allclose(got, ref, rtol=0, atol=1e-14)
