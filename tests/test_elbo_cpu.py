"""CPU: the float64 restatement of the banded operator and of UFlowElboLoss (tests/elbo_ref.py) against what the
reference's own code computed (tests/golden/elbo.npz), plus everything of the new operators and of the loss that does not
need a GPU: the raw entry points' error codes, the argument checks, the unsupported settings, get_loss."""
import ctypes

import numpy as np
import pytest
import torch

from tests import elbo_ref as R

BAND = [(tag, k, ('Y', 'gX', 'gA')) for tag, ks in R.GOLDEN_GRIDS.items() for k in ks] + \
       [(tag, 3, ('Y', 'gX')) for tag in R.GOLDEN_BIG]


def _rel(got, ref):
    scale = max(np.abs(ref).max(), 1e-300)
    return np.abs(got - ref).max() / scale


@pytest.mark.parametrize('tag,k,keep', BAND, ids=['%s-k%d' % (t, k) for t, k, _ in BAND])
def test_products_match_the_reference(golden, tag, k, keep):
    g = golden('elbo')
    M, N = R.grid_shape(tag)
    case = R.make_band_case(2, 1, M, N, k)
    assert float(g.raw('insum_%s_k%d' % (tag, k))) == sum(v.astype(np.float64).sum() for v in case.values())
    A = np.concatenate((case['diag'], case['off']), 1)
    for name, transpose in (('mv', False), ('mvT', True)):
        got = {'Y': R.product(A, case['X'], k, transpose)}
        got['gA'], got['gX'] = R.product_grads(A, case['X'], case['gY'], k, transpose)
        for key in keep:
            ref = g.raw('%s_%s_%s_k%d' % (key, name, tag, k))
            assert got[key].shape == ref.shape
            assert _rel(got[key], ref) <= 1e-12, (name, key)


@pytest.mark.parametrize('k', [0, 1, 2, 3])
@pytest.mark.parametrize('tag', list(R.GRIDS))
def test_adjoint_identity_and_sampler(tag, k):
    """<L x, g> = <x, L^T g> on every test grid (also those smaller than the band), and the sampler's folded gradients
    against the per-sample products."""
    M, N = R.GRIDS[tag]
    B, S = 2, 3
    c = R.make_band_case(B, S, M, N, k)
    A = np.tile(np.concatenate((c['diag'], c['off']), 1), (S, 1, 1, 1))
    lhs = (R.product(A, c['X'], k) * c['gY']).sum()
    rhs = (c['X'] * R.product(A, c['gY'], k, True)).sum()
    scale = (np.abs(R.product(np.abs(A), np.abs(c['X']), k)) * np.abs(c['gY'])).sum()
    assert abs(lhs - rhs) <= 1e-12 * scale
    z = R.sampler(c['mean'], c['diag'], c['off'], c['X'], k, S)
    assert np.array_equal(z[B:2 * B], c['mean'] + R.product(A[:B], c['X'][B:2 * B], k))
    gmean, gdiag, goff, gX = R.sampler_grads(c['diag'], c['off'], c['X'], c['gY'], k, S)
    gA, gX1 = R.product_grads(A, c['X'], c['gY'], k)
    assert np.array_equal(gX, gX1) and gdiag.shape == c['diag'].shape and goff.shape == c['off'].shape
    assert np.allclose(np.concatenate((gdiag, goff), 1), gA[:B] + gA[B:2 * B] + gA[2 * B:], rtol=0, atol=1e-13)
    assert np.allclose(gmean, c['gY'][:B].astype(np.float64) + c['gY'][B:2 * B] + c['gY'][2 * B:], rtol=0, atol=1e-13)


def _loss_case(g, tag):
    case = {k: g.raw('%s_%s' % (k, tag)) for k in ('net12', 'net21', 'eps12', 'eps21')}
    case.update(im1=g.raw('im1'), im2=g.raw('im2'))
    return case


@pytest.mark.parametrize('tag', list(R.CASES))
def test_loss_restatement_matches_the_reference(golden, tag):
    g = golden('elbo')
    case = _loss_case(g, tag)
    recipe = R.make_loss_case(tag)
    assert all(np.array_equal(case[k], recipe[k]) for k in case)
    got = R.loss(R.case_cfg(tag), case)
    for key in R.OUTPUTS:
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        print('%s %s: rel %.3e' % (tag, key, _rel(got[key], ref)))
        assert _rel(got[key], ref) <= 1e-12, key
    cfg = R.case_cfg(tag)
    total = got['warp'] + got['smooth'] - got['entropy'] + got['oof'] + got['occ']
    if cfg.approx == 'sparse':
        n12, n21 = case['net12'].astype(np.float64), case['net21'].astype(np.float64)
        total = total + cfg.offdiag_reg * ((n12[:, 4:] ** 2).mean() + (n21[:, 4:] ** 2).mean())
    assert abs(total - got['total']) <= 1e-12 * abs(got['total'])


# ---- the raw entry points: error codes before any launch ----------------------------------------------------------
def _fwd(lib, mean=1, diag=1, off=1, X=1, Y=1, B=2, S=2, M=4, N=5, k=1, transpose=0, bs=None):
    """Non-NULL pointers are never dereferenced: every call here must return before its launch."""
    buf = (ctypes.c_float * 4)()
    p = lambda on: ctypes.cast(buf, ctypes.c_void_p) if on else None  # noqa: E731
    bs = bs or {}
    st = lambda name, c: bs.get(name, c * M * N)  # noqa: E731
    n = (k + 1) ** 2 - 1 if 0 <= k <= 3 else 1
    return lib.arflow_band_mv_fwd(p(mean), st('mean', 2), p(diag), st('diag', 2), p(off), st('off', 2 * n), p(X), st('X', 2),
                                  p(Y), st('Y', 2), B, S, M, N, k, transpose, None)


def _bwd(lib, diag=1, off=1, X=1, gY=1, gX=1, gmean=1, gdiag=1, goff=1, B=2, S=2, M=4, N=5, k=1, transpose=0, bs=None):
    buf = (ctypes.c_float * 4)()
    p = lambda on: ctypes.cast(buf, ctypes.c_void_p) if on else None  # noqa: E731
    bs = bs or {}
    st = lambda name, c: bs.get(name, c * M * N)  # noqa: E731
    n = (k + 1) ** 2 - 1 if 0 <= k <= 3 else 1
    return lib.arflow_band_mv_bwd(p(diag), st('diag', 2), p(off), st('off', 2 * n), p(X), st('X', 2), p(gY), st('gY', 2),
                                  p(gX), st('gX', 2), p(gmean), st('gmean', 2), p(gdiag), st('gdiag', 2), p(goff),
                                  st('goff', 2 * n), B, S, M, N, k, transpose, None)


def test_raw_entry_points_reject_bad_arguments():
    from arflow_amd import _lib
    lib = _lib.load()
    assert lib.arflow_abi_version() == 10
    for name in ('diag', 'X', 'Y', 'off'):
        assert _fwd(lib, **{name: 0}) == -1001, name
    for name in ('diag', 'X', 'gY', 'gdiag', 'off', 'goff'):
        assert _bwd(lib, **{name: 0}) == -1001, name
    for call in (_fwd, _bwd):
        for dim in ('B', 'S', 'M', 'N'):
            assert call(lib, **{dim: 0}) == -1002, dim
            assert call(lib, **{dim: -3}) == -1002, dim
        for k in (-1, 4):
            assert call(lib, k=k) == -1003
        assert call(lib, transpose=2) == -1003
        assert call(lib, bs={'diag': 2 * 4 * 5 - 1}) == -1002
        assert call(lib, bs={'off': 6 * 4 * 5 - 1}) == -1002
        assert call(lib, bs={'X': 39}) == -1002
    assert _fwd(lib, bs={'mean': 39}) == -1002 and _fwd(lib, bs={'Y': 39}) == -1002
    for name in ('gY', 'gX', 'gmean', 'gdiag', 'goff'):
        assert _bwd(lib, bs={name: 39}) == -1002, name


def test_cpu_tensors_and_bad_arguments_raise():
    from arflow_amd import _lib, triag_solve as T
    A, X = torch.zeros(2, 8, 4, 5), torch.zeros(2, 2, 4, 5)
    for fn in (T.matrix_vector_product_general, T.matrix_vector_product_T_general):
        with pytest.raises(_lib.ArflowHipError, match='A is a cpu tensor'):
            fn(A, X, k=1)
        with pytest.raises(ValueError, match=r'^A must be a \[K,18,M,N\]'):
            fn(A, X, k=2)
        with pytest.raises(ValueError, match='^k must be 0..3'):
            fn(A, X, k=4)
    with pytest.raises(_lib.ArflowHipError, match='diag is a cpu tensor'):
        T.reparam_triag(X, X, A[:, :6], 1, nsamples=2)
    with pytest.raises(ValueError, match='^nsamples must be'):
        T.reparam_triag(X, X, A[:, :6], 1, nsamples=0, eps=X)
    with pytest.raises(ValueError, match='^diag must be'):
        T.reparam_triag(X, None, None, 0, eps=X)


# ---- the loss's settings ----------------------------------------------------------------------------------------
NONDIAG = {  # the loss section of the reference's configs/chairs_uflow_elbo_nondiag.json (no isotropic_smooth / order_smooth)
    'edge_constant': 150, 'edge_asymp': 0.01, 'type': 'uflow_elbo', 'w_smooth': 4.0, 'penalty_smooth': 'charbonnier',
    'closed_form_smooth': False, 'data_loss': ['census'], 'data_weight': [1.0], 'data_penalty': ['abs_robust_loss'],
    'w_entropy': 0.1, 'w_oof': 0.0, 'w_occ': 0.0, 'with_bk': True, 'approx': 'sparse', 'n_components': 1, 'cov_supp': 3,
    'inv_cov': False, 'approx_entropy': False, 'occ_type': 'sample', 'n_samples': 4, 'offdiag_reg': 0.0,
    'natural_grad': False}


def test_get_loss_and_the_shipped_nondiag_config():
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    loss = get_loss(AttrDict(NONDIAG))
    assert type(loss) is UFlowElboLoss and (loss.isotropic, loss.order, loss.closed) == (False, 1, False)
    assert type(get_loss(AttrDict(R.case_cfg('diag_closed2')))) is UFlowElboLoss


@pytest.mark.parametrize('change,match', [
    (dict(approx='mixture'), "approx: 'mixture'"), (dict(approx='lowrank'), "approx: 'lowrank'"),
    (dict(occ_type='mean'), "occ_type: 'mean'"), (dict(occ_type='none'), "occ_type: 'none'"),
    (dict(data_loss=['ssim']), r"data_loss: \['ssim'\]"), (dict(data_loss=['census', 'ssim']), 'data_loss'),
    (dict(data_penalty=['charbonnier']), r"data_penalty: \['charbonnier'\]"),
    (dict(penalty_smooth='gmm'), "penalty_smooth: 'gmm'"), (dict(penalty_smooth='identity'), "penalty_smooth: 'identity'"),
    (dict(isotropic_smooth=True), 'isotropic_smooth: True'),
    (dict(closed_form_smooth=True), "closed_form_smooth with approx: 'sparse'"),
    (dict(closed_form_smooth=True, approx='diag', order_smooth=3), 'order_smooth: 3'),
    (dict(cov_supp=4), 'cov_supp: 4'),
])
def test_unsupported_settings_raise_at_construction(change, match):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    with pytest.raises(NotImplementedError, match=match):
        UFlowElboLoss(AttrDict(dict(NONDIAG, **change)))


@pytest.mark.parametrize('change,message', [
    (dict(natural_grad=True), 'Natural gradient is not implemented!'),
    (dict(inv_cov=True), 'Sparse precision matrix representation is not implemented!')])
def test_natural_grad_and_sparse_precision_raise_as_the_reference(change, message):
    """In the forward, with the reference's words (losses/uflow_elbo_loss.py:252, :304), before anything touches a GPU."""
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    loss = UFlowElboLoss(AttrDict(dict(NONDIAG, **change)))
    net, im = torch.zeros(1, 36, 2, 2), torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError) as e:
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)
    assert str(e.value) == message


def test_loss_has_no_cpu_path():
    from arflow_amd import _lib
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    loss = UFlowElboLoss(AttrDict(NONDIAG))
    net, im = torch.zeros(1, 36, 2, 2), torch.zeros(1, 3, 8, 8)
    with pytest.raises(_lib.ArflowHipError):
        loss({'flows_fw': [None, None, net], 'flows_bw': [None, None, net]}, im, im)


def test_range_map_in_torch_matches_the_oracle_and_its_gradient():
    """The differentiable range map the w_occ term uses (plain torch) against oracle/ops.py, values and gradient."""
    from arflow_amd.losses.uflow_elbo_loss import range_map
    from oracle import ops as O
    g = torch.Generator().manual_seed(5)
    flow = (3 * torch.randn(2, 2, 6, 9, generator=g, dtype=torch.float64)).requires_grad_(True)
    w = torch.randn(2, 1, 6, 9, generator=g, dtype=torch.float64)
    a, b = range_map(flow), O.compute_range_map(flow)
    assert torch.allclose(a, b, rtol=0, atol=1e-13)
    ga, = torch.autograd.grad((a * w).sum(), flow)
    gb, = torch.autograd.grad((b * w).sum(), flow)
    assert torch.allclose(ga, gb, rtol=0, atol=1e-12)
