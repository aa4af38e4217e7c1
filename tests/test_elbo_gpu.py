"""GPU: UFlowElboLoss (arflow_amd/losses/uflow_elbo_loss.py) on every case of tests/golden/elbo.npz -- what the reference's
own loss computed in float64 on the stored inputs and the stored noise.

Bounds.  Each output is held to the larger of
  * 8 x the stored gap between the reference's OWN fp32 and float64 runs, times the output's largest magnitude (the rule
    of DESIGN.md section 16), and
  * the bound the project already applies to the same kernels in tests/test_bench_shapes_gpu.py (UFlowLoss end to end):
    5e-8 + 3e-6 |ref| for loss terms, 2e-6 + 1e-5 |ref| for masks, 2e-7 + 2e-4 max|ref| + 2e-3 |ref| for gradients.
flow12_2 is the sampler's output: the fp32 bits of the reference's order (tests/test_band_gpu.py), checked here against
float64 under the loss-term bound.  The total is recomputed from the returned terms.  `sparse3` also runs as the
per-direction composition (loss.pair = False) and must agree with the one-pass form to the bounds of
tests/test_hip_parity.py (pair vs sequential UFlowLoss: the masks for equality), and once with loss.fused = False."""
import numpy as np
import pytest
import torch

from tests import elbo_ref as R

pytestmark = pytest.mark.gpu

KIND = {'total': 'term', 'warp': 'term', 'smooth': 'term', 'entropy': 'term', 'oof': 'term', 'flow12_2': 'term',
        'occu_mask12': 'mask', 'valid_mask12': 'mask', 'gnet12': 'grad', 'gnet21': 'grad'}


def _project_bound(kind, ref):
    a = np.abs(ref)
    if kind == 'term':
        return 5e-8 + 3e-6 * a
    if kind == 'mask':
        return 2e-6 + 1e-5 * a
    return 2e-7 + 2e-4 * a.max() + 2e-3 * a


def _run(g, tag, pair=True, fused=True):
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.get_loss import get_loss
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    net12, net21 = cu('net12_' + tag).requires_grad_(True), cu('net21_' + tag).requires_grad_(True)
    loss = get_loss(AttrDict(R.case_cfg(tag)))
    loss.pair, loss.fused = pair, fused
    res = loss({'flows_fw': [None, None, net12], 'flows_bw': [None, None, net21]}, cu('im1'), cu('im2'),
               eps=(cu('eps12_' + tag), cu('eps21_' + tag)))
    g12, g21 = torch.autograd.grad(res[0], (net12, net21))
    out = dict(zip(R.OUTPUTS[:8], res))
    out.update(gnet12=g12, gnet21=g21)
    return {k: torch.as_tensor(v).detach().double().cpu().numpy() for k, v in out.items()}, (net12, net21)


@pytest.fixture(scope='module')
def runs(golden):
    """runs(tag): the case through the default path, computed when first asked for and then shared."""
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = _run(golden('elbo'), tag)
        return cache[tag]
    return get


def _against_the_reference(g, tag, got):
    bad = []
    for key in R.OUTPUTS:
        ref = g.raw('%s_%s' % (key, tag))
        assert got[key].shape == ref.shape, key
        bound = np.maximum(8 * float(g.raw('noise_%s_%s' % (key, tag))) * np.abs(ref).max(), _project_bound(KIND[key], ref))
        err = np.abs(got[key] - ref)
        print('%s %-12s max err %.3e  max err / bound %.3f  max|ref| %.3e' % (tag, key, err.max(), (err / bound).max(),
                                                                              np.abs(ref).max()))
        if not (np.isfinite(got[key]).all() and (err <= bound).all()):
            bad.append(key)
    assert not bad, bad


@pytest.mark.parametrize('tag', list(R.CASES))
def test_loss_against_the_reference(golden, runs, tag):
    g = golden('elbo')
    got, nets = runs(tag)
    _against_the_reference(g, tag, got)
    # the total, recomputed from the returned terms in float64 (the occlusion penalty is not returned: w_occ = 0 here)
    cfg = R.case_cfg(tag)
    if cfg.w_occ == 0:
        total = got['warp'] + got['smooth'] - got['entropy'] + got['oof']
        if cfg.approx == 'sparse':
            off = [n.detach()[:, 4:].double() for n in nets]
            total = total + cfg.offdiag_reg * float((off[0] ** 2).mean() + (off[1] ** 2).mean())
        assert abs(total - got['total']) <= 5e-8 + 3e-6 * abs(total)


def test_occlusion_penalty_is_the_rest_of_the_total(golden, runs):
    """w_occ > 0: total - (warp + smooth - entropy + oof) is the occlusion penalty of the restatement."""
    tag = 'nobk_oof_occ'
    g = golden('elbo')
    got, _ = runs(tag)
    case = {k: g.raw('%s_%s' % (k, tag)) for k in ('net12', 'net21', 'eps12', 'eps21')}
    case.update(im1=g.raw('im1'), im2=g.raw('im2'))
    occ = float(R.loss(R.case_cfg(tag), case)['occ'])
    rest = got['total'] - (got['warp'] + got['smooth'] - got['entropy'] + got['oof'])
    assert occ > 0 and abs(rest - occ) <= 5e-8 + 3e-6 * abs(got['total'])


def test_one_pass_form_equals_the_per_direction_composition(golden, runs):
    from arflow_amd import functional as AF
    g = golden('elbo')
    launched = {}
    for pair in (True, False):  # the switch selects the path: the launches say which one ran
        AF.start_kernel_timing()
        res, _ = _run(g, 'sparse3', pair=pair)
        launched[pair] = {name for name, _ in AF.stop_kernel_timing()}
        if not pair:
            seq = res
    assert 'arflow_uflow_pair_bwd' in launched[True] and 'arflow_census_warp_bwd' not in launched[True]
    assert 'arflow_census_warp_bwd' in launched[False] and 'arflow_uflow_pair_bwd' not in launched[False]
    assert {'arflow_band_mv_fwd', 'arflow_band_mv_bwd'} <= launched[True] & launched[False]
    pair, _ = runs('sparse3')
    for key in R.SCALARS:
        err = abs(pair[key] - seq[key])
        print('%s: %.3e' % (key, err))
        assert err <= 1e-7 + 2e-6 * abs(seq[key]), key
    for key in ('flow12_2', 'valid_mask12', 'occu_mask12'):
        print('%s: %d elements differ' % (key, int((pair[key] != seq[key]).sum())))
        assert np.array_equal(pair[key], seq[key]), key
    for key in ('gnet12', 'gnet21'):
        err = np.abs(pair[key] - seq[key])
        assert (err <= 1e-7 * np.abs(seq[key]).max() + 1e-12 + 1e-5 * np.abs(seq[key])).all(), (key, float(err.max()))


def test_unfused_photometric_path_against_the_reference(golden):
    """loss.fused = False: x1/4 copies without grey planes, the S-fold image repeat, warp, mask upsample and census as
    separate launches, per direction -- `sparse3` against the fixture under the bounds of the default path."""
    from arflow_amd import functional as AF
    g = golden('elbo')
    AF.start_kernel_timing()
    got, _ = _run(g, 'sparse3', fused=False)
    launched = {name for name, _ in AF.stop_kernel_timing()}
    assert {'arflow_down4', 'arflow_warp_fwd', 'arflow_up4_clamp_mul', 'arflow_census_fwd'} <= launched, launched
    assert not launched & {'arflow_uflow_pair_bwd', 'arflow_census_warp_fwd', 'arflow_down4_gray_z'}, launched
    _against_the_reference(g, 'sparse3', got)


def test_noise_is_drawn_on_the_device_and_deterministic_mode_reproduces(golden):
    """eps=None: two calls differ; with the stored noise, two calls in deterministic mode agree bit for bit, loss and
    gradients."""
    from arflow_amd import functional as AF
    from arflow_amd.config import AttrDict
    from arflow_amd.losses.uflow_elbo_loss import UFlowElboLoss
    g = golden('elbo')
    tag = 'sparse3'
    cu = lambda name: torch.from_numpy(np.array(g.raw(name))).cuda()  # noqa: E731
    loss = UFlowElboLoss(AttrDict(R.case_cfg(tag)))
    nets = {'flows_fw': [None, None, cu('net12_' + tag)], 'flows_bw': [None, None, cu('net21_' + tag)]}
    a, b = loss(nets, cu('im1'), cu('im2')), loss(nets, cu('im1'), cu('im2'))
    assert a[5].shape == (4, 2, 8, 16) and bool(torch.isfinite(a[0])) and not torch.equal(a[5], b[5])
    with AF.deterministic():
        one, _ = _run(g, tag)
        two, _ = _run(g, tag)
    for key in R.OUTPUTS:
        assert np.array_equal(one[key], two[key]), key
