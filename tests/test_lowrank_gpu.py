"""GPU: the kernels of csrc/lowrank.hip (sampler, Gram log-determinant, backward) and the autograd node of
arflow_amd/lowrank.py against the float64 restatement of tests/lowrank_ref.py.

Bounds, derived (the rule of tests/test_band_gpu.py): an fp32 sum of `terms` rounded products, added in a fixed order, is
within (terms + 2) 2^-24 sum |term| of the exact value per element.
  sampler forward   terms = R + 1 (the mean and R products)
  gmean             terms = S
  gstd              terms = S + R (S products of the sampler's adjoint, R of the log-det's; the fp32 rounding of G^-1 the
                    kernel reads is one more rounding on each of the R terms and the factor 2 glogdet is exact)
  logdet            2 * 2^-24 max(|ref|, 1): a float64 computation on exact inputs, rounded once
  ginv              4 * 2^-24 max |ref| per matrix
Every case asserts cond(G) < 1e4 on the float64 reference, so no bound hides a rank problem.

Grids: a single pixel (R = 1), 2 x 3 (R <= 3), odd 17 x 23 (M N % 4 != 0: the scalar-load path of stage 1), 8 x 33 and 9 x 32 (M N
% 4 == 0: the float4 path, with a ragged last trip), and two grids of more than two stage-1 chunks (lowrank_ref.CHUNK = 1024
pixels per workgroup) with a ragged last one: 36 x 60 = 2160 pixels on the float4 path and 33 x 65 = 2145 on the scalar path.
Inputs are channel slices of one wider tensor, outputs channel slices of NaN-filled wider tensors."""
import numpy as np
import pytest
import torch

from tests import lowrank_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
BIG_VEC, BIG_ODD = (36, 60), (33, 65)
assert 2 * R.CHUNK < BIG_VEC[0] * BIG_VEC[1] < 3 * R.CHUNK and BIG_VEC[0] * BIG_VEC[1] % 4 == 0
assert 2 * R.CHUNK < BIG_ODD[0] * BIG_ODD[1] < 3 * R.CHUNK and BIG_ODD[0] * BIG_ODD[1] % 4 != 0
GRIDS = {'one': (1, 1), 'tiny': (2, 3), 'odd': (17, 23), 'wider': (8, 33), 'taller': (9, 32), 'chunks': BIG_VEC,
         'chunks_odd': BIG_ODD}
RS = (1, 3, 15, 16)
SHAPES = [(tag, r) for tag, (M, N) in GRIDS.items() for r in RS
          if M * N >= r and (tag != 'one' or r == 1) and (tag != 'tiny' or r <= 3)]
BATCHES = [(2, 1), (2, 3), (3, 1)]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(parts, pad=1):
    """Channel slices of ONE wider NaN-padded tensor: [pad | parts... | pad] -> the slices."""
    n, _, M, N = parts[0].shape
    C = sum(p.shape[1] for p in parts) + 2 * pad
    wide = torch.full((n, C, M, N), float('nan'), device='cuda')
    out, c = [], pad
    for p in parts:
        wide[:, c:c + p.shape[1]] = p
        out.append(wide[:, c:c + p.shape[1]])
        c += p.shape[1]
    return wide, out


def _nan_slice(n, C, M, N, pad=1):
    wide = torch.full((n, C + 2 * pad, M, N), float('nan'), device='cuda')
    return wide, wide[:, pad:pad + C]


def _pads_untouched(wide, pad=1):
    return bool(torch.isnan(wide[:, :pad]).all() and torch.isnan(wide[:, -pad:]).all())


_REF = {}


def _reference(B, S, r, M, N):
    """The case and its float64 results, computed once per shape and left unchanged."""
    key = (B, S, r, M, N)
    if key not in _REF:
        c = R.make_case(B, S, r, M, N)
        ref = {'case': c}
        ref['z'], ref['z_mag'] = R.sampler(c['mean'], c['std'], c['eps'], S)
        G = R.gram(c['std'])
        ref['cond'] = float(np.linalg.cond(G).max())
        ref['logdet'], ref['ginv'] = R.logdet(c['std'])
        for name, gz, gl in (('gz', c['gZ'], None), ('gl', None, c['glogdet']), ('both', c['gZ'], c['glogdet'])):
            ref[name] = R.grads(c['std'], c['eps'], gz, gl, S)
        _REF[key] = ref
    return _REF[key]


def _check(name, got, ref, bound):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, name
    err = np.abs(got - ref)
    ratio = err / np.maximum(bound, 1e-300)
    print('%-10s max err %.3e  max err / bound %.3f' % (name, err.max(), np.where(err > 0, ratio, 0.).max()))
    assert np.isfinite(got).all() and (err <= bound).all(), name


def _run_kernels(ref, B, S, r, M, N, offset=0):
    """All three entry points on channel slices, outputs into NaN-filled slices.  offset: floats the input tensor is shifted
    off its allocation's alignment by.  -> dict of results (the tensors the kernels wrote)."""
    from arflow_amd import lowrank as LR
    c = ref['case']
    if offset:
        flat = torch.full((B * (2 + 2 * r + 2) * M * N + offset,), float('nan'), device='cuda')
        net_wide = flat[offset:].view(B, 2 + 2 * r + 2, M, N)
        net_wide[:, 1:3], net_wide[:, 3:3 + 2 * r] = _cuda(c['mean']), _cuda(c['std'])
        mean, std = net_wide[:, 1:3], net_wide[:, 3:3 + 2 * r]
    else:
        net_wide, (mean, std) = _wide([_cuda(c['mean']), _cuda(c['std'])])
    eps, gZ_wide, glogdet = _cuda(c['eps']), _wide([_cuda(c['gZ'])]), _cuda(c['glogdet'])
    gZ = gZ_wide[1][0]
    out = {}
    z_wide, z = _nan_slice(S * B, 2, M, N)
    LR._sample_fwd(mean, std, eps, S, z)
    assert _pads_untouched(z_wide)
    out['z'] = z
    ld = torch.full((B, 2), float('nan'), device='cuda')
    ginv = torch.full((B, 2, r, r), float('nan'), device='cuda')
    LR._logdet_fwd(std, logdet=ld, ginv=ginv)
    out['logdet'], out['ginv'] = ld, ginv
    for name, gz, gl in (('gz', gZ, None), ('gl', None, glogdet), ('both', gZ, glogdet)):
        g_wide, g = _nan_slice(B, 2 + 2 * r, M, N)
        LR._bwd(std, eps, gz, ginv, gl, S, True, gmean=g[:, 0:2], gstd=g[:, 2:])
        assert _pads_untouched(g_wide)
        out[name] = g
    return out


def _against_the_reference(ref, got, B, S, r):
    assert ref['cond'] < 1e4, ref['cond']
    _check('z', got['z'], ref['z'], (r + 1 + 2) * EPS * ref['z_mag'])
    _check('logdet', got['logdet'], ref['logdet'], 2 * EPS * np.maximum(np.abs(ref['logdet']), 1.0))
    _check('ginv', got['ginv'], ref['ginv'], 4 * EPS * np.abs(ref['ginv']).max(axis=(2, 3), keepdims=True) * np.ones_like(ref['ginv']))
    for name in ('gz', 'gl', 'both'):
        gmean, gstd, mag_mean, mag_std = ref[name]
        _check(name + ' gmean', got[name][:, 0:2], gmean, (S + 2) * EPS * mag_mean)
        _check(name + ' gstd', got[name][:, 2:], gstd, (S + r + 2) * EPS * mag_std)


@pytest.mark.parametrize('B,S', BATCHES, ids=['B%dS%d' % bs for bs in BATCHES])
@pytest.mark.parametrize('tag,r', SHAPES, ids=['%s-R%d' % s for s in SHAPES])
def test_kernels_against_float64(tag, r, B, S):
    M, N = GRIDS[tag]
    ref = _reference(B, S, r, M, N)
    _against_the_reference(ref, _run_kernels(ref, B, S, r, M, N), B, S, r)


@pytest.mark.parametrize('r', [3, 16])
def test_misaligned_planes_take_the_scalar_path(r):
    """9 x 32 has M N % 4 == 0, but the tensor starts one float off a 16-byte boundary: float4 loads would fault or read the
    wrong pixels."""
    B, S, (M, N) = 2, 1, GRIDS['taller']
    ref = _reference(B, S, r, M, N)
    _against_the_reference(ref, _run_kernels(ref, B, S, r, M, N, offset=1), B, S, r)


@pytest.mark.parametrize('tag,r', [('odd', 15), ('chunks', 16), ('chunks_odd', 3)])
def test_repeats_agree_bit_for_bit_in_both_modes(tag, r):
    from arflow_amd import functional as AF
    B, S, (M, N) = 2, 3, GRIDS[tag]
    ref = _reference(B, S, r, M, N)
    runs = [_run_kernels(ref, B, S, r, M, N) for _ in range(2)]
    with AF.deterministic():
        runs += [_run_kernels(ref, B, S, r, M, N) for _ in range(2)]
    for other in runs[1:]:
        for key, v in runs[0].items():
            assert torch.equal(v, other[key]), key


@pytest.mark.parametrize('r,S', [(3, 2), (15, 1)])
def test_autograd_node_against_float64(r, S):
    """reparam_lowrank_pair on channel slices of the two level-2 outputs: one sampler launch and one log-det call per direction
    forward, ONE arflow_lowrank_bwd per direction backward, gradients of sum(gZ z) + sum(glogdet logdet) for the whole nets;
    then reparam_lowrank and gram_logdet alone (one source each)."""
    from arflow_amd import functional as AF, lowrank as LR
    B, (M, N) = 2, GRIDS['odd']
    ref0 = _reference(B, S, r, M, N)
    cases = [ref0['case'], R.make_case(B, S, r, M, N, seed=29)]  # the second direction: another draw
    nets = [torch.cat((_cuda(c['mean']), _cuda(c['std'])), 1).requires_grad_(True) for c in cases]
    AF.start_kernel_timing()
    flows, ld = LR.reparam_lowrank_pair(*[(n[:, 0:2], n[:, 2:], _cuda(c['eps'])) for n, c in zip(nets, cases)], S)
    gz = torch.cat([_cuda(c['gZ']) for c in cases], 1)
    gl = torch.stack([_cuda(c['glogdet']) for c in cases])
    g = torch.autograd.grad((flows, ld), nets, (gz, gl))
    launched = AF.stop_kernel_timing()
    count = lambda n: sum(len(v) for (name, _), v in launched.items() if name == n)  # noqa: E731
    assert (count('arflow_lowrank_sample_fwd'), count('arflow_lowrank_logdet_fwd'), count('arflow_lowrank_bwd')) == (2, 2, 2)
    assert flows.shape == (S * B, 4, M, N) and ld.shape == (2, B, 2)
    for d, c in enumerate(cases):
        z, mag = R.sampler(c['mean'], c['std'], c['eps'], S)
        _check('z', flows[:, 2 * d:2 * d + 2], z, (r + 3) * EPS * mag)
        ref_ld = R.logdet(c['std'])[0]
        _check('logdet', ld[d], ref_ld, 2 * EPS * np.maximum(np.abs(ref_ld), 1.0))
        gmean, gstd, mag_mean, mag_std = R.grads(c['std'], c['eps'], c['gZ'], c['glogdet'], S)
        _check('gmean', g[d][:, 0:2], gmean, (S + 2) * EPS * mag_mean)
        _check('gstd', g[d][:, 2:], gstd, (S + r + 2) * EPS * mag_std)
    c, net = cases[0], nets[0]
    z = LR.reparam_lowrank(net[:, 0:2], net[:, 2:], S, eps=_cuda(c['eps']))
    assert torch.equal(z, flows[:, 0:2])
    (g1,) = torch.autograd.grad(z, net, _cuda(c['gZ']))
    gmean, gstd, mag_mean, mag_std = ref0['gz']
    _check('gmean', g1[:, 0:2], gmean, (S + 2) * EPS * mag_mean)
    _check('gstd', g1[:, 2:], gstd, (S + r + 2) * EPS * mag_std)
    one = LR.gram_logdet(net[:, 2:])
    assert torch.equal(one, ld[0])
    (g2,) = torch.autograd.grad(one, net, _cuda(c['glogdet']))
    _, gstd, _, mag_std = ref0['gl']
    assert not g2[:, 0:2].any()
    _check('gstd', g2[:, 2:], gstd, (S + r + 2) * EPS * mag_std)
    a, b = LR.reparam_lowrank(net[:, 0:2], net[:, 2:], S), LR.reparam_lowrank(net[:, 0:2], net[:, 2:], S)
    assert a.shape == (S * B, 2, M, N) and not torch.equal(a, b)  # the noise is drawn on the device


def test_too_few_pixels_raise():
    from arflow_amd import lowrank as LR
    with pytest.raises(ValueError, match='cannot carry 3 independent columns'):
        LR.gram_logdet(torch.zeros(1, 6, 1, 2, device='cuda'))
