"""GPU: the kernels of csrc/mixture.hip (sampler + partial sums, log-density, backward, entropy map) and the autograd node of
arflow_amd/mixture.py against the float64 restatement of tests/mixture_ref.py.

Bounds, derived (tests/mixture_ref.py states the kernels' arithmetic and defines the magnitudes; EPS = 2^-24):
  samples    4 EPS (|mean_z| + |std_z eps|) per element: 1 ulp of expf, the product's rounding, the sum's rounding
  logpdf     8 EPS sum |terms| / P (mixture_ref.logpdf_bound): the terms of A are float64 from the first addition on, so what
             is left is the fp32 exponential inside d, the sample's own rounding carried through (flow - mean_k) / std_k (the
             restatement evaluates the density at ITS float64 sample, so that term belongs to the sum), and one final rounding
  resp, q    the bound on A times the softmax sensitivities r_k |delta_kj - r_j|, summed over the components, plus 4 EPS
             (mixture_ref.resp_bound)
  gradients  8 EPS sum_s |terms| per element (every product of the backward, with the sample-rounding term of each; the kernel
             adds them in float64 and rounds once) plus sum |d gradient / d r[n,j]| times the resp bound: the backward reads the
             fp32 responsibilities the forward stored
  gweights   sum_s |glogpdf[n]| (q bound)[n,k] / P + (S + 2) EPS sum_s |glogpdf[n] q[n,k]| / P: an fp32 product and sum in torch
  entropy    8 EPS (1 / n) sum_i sum_k r_k |terms of x_k| per pixel (mixture_ref.entropy_map)

Shapes (B, S, K, h x w): degenerate sizes; 3 x 5, the scalar tail only (no float4 group); 8 x 16 with K = KMAX on the float4
path; 40 x 52 = 2080 pixels = two full sampler chunks (mixture_ref.CHUNK = 1024) and a ragged third, on the float4 path when
contiguous; and 41 x 51 = 2091 on the scalar path.  Every shape runs once on contiguous tensors and once with mean and log_std
as channel slices of ONE [B,4K+3,h,w] tensor (whose planes are 16-byte aligned only when h w % 4 == 0), all outputs into channel
slices of NaN-filled wider tensors."""
import numpy as np
import pytest
import torch

from tests import mixture_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 3, 5), (2, 2, 4, 8, 16), (1, 3, 3, 40, 52), (1, 2, 2, 41, 51)]
assert 2 * R.CHUNK < 40 * 52 < 3 * R.CHUNK and 40 * 52 % 4 == 0 and 2 * R.CHUNK < 41 * 51 < 3 * R.CHUNK and 41 * 51 % 4
MODES = [('mixed', 'uniform'), ('equal', 'nonuniform'), ('mixed', 'zero')]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan_slice(n, C, M, N, pad=1):
    wide = torch.full((n, C + 2 * pad, M, N), float('nan'), device='cuda')
    return wide, wide[:, pad:pad + C]


def _pads_untouched(wide, pad=1):
    return bool(torch.isnan(wide[:, :pad]).all() and torch.isnan(wide[:, -pad:]).all())


_REF = {}


def _reference(B, S, K, M, N, comp='mixed', weights='uniform'):
    """The case and its float64 results, computed once per shape and mode and left unchanged."""
    key = (B, S, K, M, N, comp, weights)
    if key not in _REF:
        c = R.make_case(B, S, K, M, N, comp=comp, weights=weights)
        a = (c['mean'], c['log_std'], c['weights'], c['comp'], c['eps'])
        den = R.density(*a, S)
        rb = R.resp_bound(den)
        ref = {'case': c, 'den': den, 'rb': rb, 'qb': R.resp_bound(den, q=True)}
        for name, gz, gl in (('gz', c['gZ'], None), ('gl', None, c['glogpdf']), ('both', c['gZ'], c['glogpdf'])):
            ref[name] = R.grads(*a, gz, gl, S, rb=rb)
        _REF[key] = ref
    return _REF[key]


def _check(name, got, ref, bound):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, name
    err = np.abs(got - ref)
    ratio = err / np.maximum(bound, 1e-300)
    print('%-14s max err %.3e  max err / bound %.3f' % (name, err.max(), np.where(err > 0, ratio, 0.).max()))
    assert np.isfinite(got).all() and (err <= bound).all(), name


def _inputs(c, sliced):
    """mean, log_std: contiguous, or channel slices [1:1+2K] and [2+2K:2+4K] of one NaN-filled [B,4K+3,M,N] tensor."""
    B, C, M, N = c['mean'].shape
    if not sliced:
        return _cuda(c['mean']), _cuda(c['log_std'])
    wide = torch.full((B, 2 * C + 3, M, N), float('nan'), device='cuda')
    wide[:, 1:1 + C], wide[:, 2 + C:2 + 2 * C] = _cuda(c['mean']), _cuda(c['log_std'])
    return wide[:, 1:1 + C], wide[:, 2 + C:2 + 2 * C]


def _run_kernels(ref, S, sliced):
    """All entry points of the node; every image-like output goes into a channel slice of a NaN-filled wider tensor.
    -> dict of results (the tensors the kernels wrote)."""
    from arflow_amd import mixture as MX
    c = ref['case']
    B, C, M, N = c['mean'].shape
    mean, log_std = _inputs(c, sliced)
    weights, comp, eps, glp = _cuda(c['weights']), _cuda(c['comp']), _cuda(c['eps']), _cuda(c['glogpdf'])
    gz_wide, gZ = _nan_slice(S * B, 2, M, N)
    gZ.copy_(_cuda(c['gZ']))
    out = {}
    z_wide, z = _nan_slice(S * B, 2, M, N)
    out['logpdf'], out['resp'], out['q'] = MX._sample_fwd(mean, log_std, weights, comp, eps, S, z)
    assert _pads_untouched(z_wide)
    out['flow'] = z
    for name, gz, gl in (('gz', gZ, None), ('gl', None, glp), ('both', gZ, glp)):
        g_wide, g = _nan_slice(B, 2 * C, M, N)
        MX._bwd(mean, log_std, comp, eps, out['resp'], gl, gz, S, gmean=g[:, :C], glog_std=g[:, C:])
        assert _pads_untouched(g_wide)
        out[name] = g
    return out


def _against_the_reference(ref, got, S):
    den = ref['den']
    B, C, M, N = ref['case']['mean'].shape
    _check('flow', got['flow'], den['flow'], 4 * EPS * den['fmag'])
    _check('logpdf', got['logpdf'], den['logpdf'], R.logpdf_bound(den, M * N))
    _check('resp', got['resp'], den['resp'], ref['rb'])
    _check('q', got['q'], den['q'], ref['qb'])
    for name in ('gz', 'gl', 'both'):
        r = ref[name]
        _check(name + ' gmean', got[name][:, :C], r['gmean'], 8 * EPS * r['mag_mean'] + r['rs_mean'])
        _check(name + ' glog_std', got[name][:, C:], r['glog_std'], 8 * EPS * r['mag_ls'] + r['rs_ls'])


@pytest.mark.parametrize('comp,weights', MODES, ids=['%s-%s' % m for m in MODES])
@pytest.mark.parametrize('B,S,K,M,N', SHAPES, ids=['B%dS%dK%d-%dx%d' % s for s in SHAPES])
def test_kernels_against_float64(B, S, K, M, N, comp, weights):
    ref = _reference(B, S, K, M, N, comp, weights)
    r = ref['den']['resp']
    if K > 1:
        if weights == 'zero':
            assert (r[:, K - 1] == 0).all() and (ref['case']['weights'][:, K - 1] == 0).all()
        else:
            assert float(np.minimum(r, 1 - r).max()) > 0.05, 'the case does not exercise the cross-component terms'
    for sliced in (False, True):
        got = _run_kernels(ref, S, sliced)
        _against_the_reference(ref, got, S)
        if K > 1 and weights == 'zero':
            assert not got['resp'][:, K - 1].any() and bool(torch.isfinite(got['q']).all())


def test_one_component_is_the_diagonal_sampler():
    """K = 1, comp = 0: the samples are mean + exp(log_std) eps, the responsibilities 1, and gmean = sum_s gZ: the two routes of
    the density's gradient into the mean cancel (to the gradient bound; the kernel adds both in float64)."""
    B, S, K, M, N = 2, 3, 1, 3, 5
    ref = _reference(B, S, K, M, N, 'equal', 'uniform')
    c = ref['case']
    assert not c['comp'].any()
    got = _run_kernels(ref, S, False)
    z = np.tile(c['mean'].astype(np.float64), (S, 1, 1, 1)) + np.exp(np.tile(c['log_std'].astype(np.float64), (S, 1, 1, 1))) * c['eps']
    _check('flow', got['flow'], z, 4 * EPS * ref['den']['fmag'])
    assert bool((got['resp'] == 1).all()) and bool((got['q'] == 1).all())
    fold = sum(c['gZ'][s * B:(s + 1) * B].astype(np.float64) for s in range(S))
    r = ref['both']
    _check('gmean', got['both'][:, :2], fold, 8 * EPS * r['mag_mean'] + r['rs_mean'])


def test_misaligned_planes_take_the_scalar_path():
    """8 x 16 has h w % 4 == 0, but the tensors start one float off a 16-byte boundary: float4 loads would fault or read the
    wrong pixels."""
    from arflow_amd import mixture as MX
    B, S, K, M, N = 2, 2, 4, 8, 16
    ref = _reference(B, S, K, M, N)
    c = ref['case']

    def shifted(a):
        flat = torch.full((a.size + 1,), float('nan'), device='cuda')
        flat[1:] = _cuda(a).reshape(-1)
        return flat[1:].view(a.shape)
    mean, log_std, eps = shifted(c['mean']), shifted(c['log_std']), shifted(c['eps'])
    assert mean.data_ptr() % 16 == 4
    z = torch.full((S * B, 2, M, N), float('nan'), device='cuda')
    lp, _, _ = MX._sample_fwd(mean, log_std, _cuda(c['weights']), _cuda(c['comp']), eps, S, z)
    _check('flow', z, ref['den']['flow'], 4 * EPS * ref['den']['fmag'])
    _check('logpdf', lp, ref['den']['logpdf'], R.logpdf_bound(ref['den'], M * N))


@pytest.mark.parametrize('shape', [(2, 3, 2, 3, 5), (1, 3, 3, 40, 52)], ids=['3x5', '40x52'])
def test_repeats_agree_bit_for_bit_in_both_modes(shape):
    from arflow_amd import functional as AF
    B, S, K, M, N = shape
    ref = _reference(B, S, K, M, N)
    runs = [_run_kernels(ref, S, True) for _ in range(2)]
    with AF.deterministic():
        runs += [_run_kernels(ref, S, True) for _ in range(2)]
    for other in runs[1:]:
        for key, v in runs[0].items():
            assert torch.equal(v, other[key]), key


def test_autograd_node_against_float64():
    """reparam_gmm_pair on the two level-2 outputs (means then log-stds) with weights that require grad: one sampler and one
    log-density launch per direction forward, ONE arflow_mixture_bwd per direction backward, gradients of sum(gZ flow) +
    sum(glogpdf logpdf) for the whole nets and the weights; then reparam_gmm and gaussian_mixture_log_pdf alone."""
    from arflow_amd import functional as AF, mixture as MX
    B, S, K, M, N = 2, 3, 2, 3, 5
    refs = [_reference(B, S, K, M, N, 'mixed', 'nonuniform'), _reference(B, S, K, M, N, 'equal', 'nonuniform')]
    cases = [r['case'] for r in refs]
    nets = [torch.cat((_cuda(c['mean']), _cuda(c['log_std'])), 1).requires_grad_(True) for c in cases]
    ws = [_cuda(c['weights']).requires_grad_(True) for c in cases]
    AF.start_kernel_timing()
    flows, lp = MX.reparam_gmm_pair(*[(n, w, _cuda(c['comp']), _cuda(c['eps'])) for n, w, c in zip(nets, ws, cases)], S)
    gz = torch.cat([_cuda(c['gZ']) for c in cases], 1)
    gl = torch.stack([_cuda(c['glogpdf']) for c in cases])
    g = torch.autograd.grad((flows, lp), nets + ws, (gz, gl))
    launched = AF.stop_kernel_timing()
    count = lambda n: sum(len(v) for (name, _), v in launched.items() if name == n)  # noqa: E731
    assert (count('arflow_mixture_sample_fwd'), count('arflow_mixture_logpdf_fwd'), count('arflow_mixture_bwd')) == (2, 2, 2)
    assert flows.shape == (S * B, 4, M, N) and lp.shape == (2, S * B)
    for d, ref in enumerate(refs):
        den, r = ref['den'], ref['both']
        _check('flow', flows[:, 2 * d:2 * d + 2], den['flow'], 4 * EPS * den['fmag'])
        _check('logpdf', lp[d], den['logpdf'], R.logpdf_bound(den, M * N))
        _check('gmean', g[d][:, :2 * K], r['gmean'], 8 * EPS * r['mag_mean'] + r['rs_mean'])
        _check('glog_std', g[d][:, 2 * K:], r['glog_std'], 8 * EPS * r['mag_ls'] + r['rs_ls'])
        gq = np.abs(cases[d]['glogpdf'].astype(np.float64))[:, None] * ref['qb'] / (M * N)
        _check('gweights', g[2 + d], r['gweights'], gq.reshape(S, B, K).sum(0) + (S + 2) * EPS * r['mag_w'])
    c, net, w = cases[0], nets[0], ws[0]
    z = MX.reparam_gmm(net[:, :2 * K], net[:, 2 * K:], w, S, comp=_cuda(c['comp']), eps=_cuda(c['eps']))
    assert torch.equal(z, flows[:, 0:2])
    (g1,) = torch.autograd.grad(z, net, _cuda(c['gZ']))
    r = refs[0]['gz']
    _check('gmean', g1[:, :2 * K], r['gmean'], 8 * EPS * r['mag_mean'] + r['rs_mean'])
    _check('glog_std', g1[:, 2 * K:], r['glog_std'], 8 * EPS * r['mag_ls'] + r['rs_ls'])
    z2, lp2 = MX.gaussian_mixture_log_pdf(None, net[:, :2 * K], net[:, 2 * K:], w, S, comp=_cuda(c['comp']), eps=_cuda(c['eps']))
    assert torch.equal(z2, z) and lp2.shape == (S * B, 1) and torch.equal(lp2[:, 0], lp[0])
    g2 = torch.autograd.grad(lp2, (net, w), _cuda(c['glogpdf']).unsqueeze(1))
    r = refs[0]['gl']
    _check('gmean', g2[0][:, :2 * K], r['gmean'], 8 * EPS * r['mag_mean'] + r['rs_mean'])
    _check('glog_std', g2[0][:, 2 * K:], r['glog_std'], 8 * EPS * r['mag_ls'] + r['rs_ls'])


def test_draws_on_the_device():
    """eps=None, comp=None: two calls differ and are finite; the drawn components stay in 0..K-1 and never take a component of
    weight zero."""
    from arflow_amd import mixture as MX
    B, S, K, M, N = 2, 8, 3, 3, 5
    c = R.make_case(B, S, K, M, N, weights='zero')
    mean, log_std, w = _cuda(c['mean']), _cuda(c['log_std']), _cuda(c['weights'])
    a, b = MX.reparam_gmm(mean, log_std, w, S), MX.reparam_gmm(mean, log_std, w, S)
    assert a.shape == (S * B, 2, M, N) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert not torch.equal(a, b)
    comp, eps = MX._draw(mean, w, 64, None, None)
    assert comp.shape == (B, 64) and comp.dtype == torch.int64 and comp.is_cuda and eps.shape == (64 * B, 2, M, N)
    assert int(comp.min()) >= 0 and int(comp.max()) <= K - 2
    e1, e2 = MX.mixture_entropy(mean, log_std, w, 7), MX.mixture_entropy(mean, log_std, w, 7)
    assert e1.shape == (B, 1, M, N) and e1.is_cuda and bool(torch.isfinite(e1).all()) and not torch.equal(e1, e2)


def test_entropy_map_against_the_reference_fixture(golden):
    from arflow_amd import mixture as MX
    g = golden('elbo_mixture')
    c = {k: g.raw(k + '_entropy_map') for k in ('mean', 'log_std', 'weights', 'comp', 'eps')}
    n = R.ENTROPY_N
    _, mag = R.entropy_map(c['mean'], c['log_std'], c['weights'], c['comp'], c['eps'], n)
    got = MX.mixture_entropy(_cuda(c['mean']), _cuda(c['log_std']), _cuda(c['weights']), n, comp=_cuda(c['comp']), eps=_cuda(c['eps']))
    ref = g.raw('out_entropy_map')
    _check('entropy', got, ref, 8 * EPS * mag + 1e-10 * np.abs(ref).max())


@pytest.mark.parametrize('B,n,K,M,N,weights', [(2, 3, 2, 3, 5, 'uniform'), (1, 3, 3, 40, 52, 'nonuniform'), (2, 2, 4, 8, 16, 'zero')],
                         ids=['3x5', '40x52', '8x16-zero'])
def test_entropy_map_against_float64(B, n, K, M, N, weights):
    from arflow_amd import mixture as MX
    c = _reference(B, n, K, M, N, 'mixed', weights)['case']
    ref, mag = R.entropy_map(c['mean'], c['log_std'], c['weights'], c['comp'], c['eps'], n)
    for sliced in (False, True):
        mean, log_std = _inputs(c, sliced)
        got = MX.mixture_entropy(mean, log_std, _cuda(c['weights']), n, comp=_cuda(c['comp']), eps=_cuda(c['eps']))
        _check('entropy', got, ref, 8 * EPS * mag)
    again = MX.mixture_entropy(mean, log_std, _cuda(c['weights']), n, comp=_cuda(c['comp']), eps=_cuda(c['eps']))
    assert torch.equal(got, again)
