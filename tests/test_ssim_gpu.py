"""The stand-alone photometric kernels (csrc/ssim.hip) off their fixture sizes: the 1-px and the 4-px tilings at their
minimum, on partial tiles and across tile edges, against the CPU oracle (oracle.ops.ssim, plain torch for L1).

  (1, 1, 3, 3)     1-px path (W % 4 != 0), a single window
  (2, 3, 11, 35)   1-px path, crosses the 8-row and the 32-column tile edge; the last tile is 3 columns wide
  (1, 2, 3, 4)     4-px path (W % 4 == 0) at its minimum
  (2, 3, 19, 68)   4-px path, crosses the 16-row and the 64-column edge: last tile column one lane group, last tile row 3 rows
  (1, 3, 17, 128)  4-px path, exactly two tiles wide, a one-row second tile row

Per shape: (a) the three sums of PhotoSumsFunction and d / d recons of 0.3 s0 + 0.7 s1, with a random 0/1 mask and with
mask=None; (b) the SSIM map of loss_blocks.SSIM and both gradients under a random upstream map (the `gmap` branch of the
backward kernels, which the sums never take).

Tolerances are the project's: the map and its gradients as test_photo_blocks_golden (sigma = E[x^2] - mu^2 cancels
against C2 = 9e-4, which amplifies fp32 rounding ~1e3 x), d / d recons as test_photometric_sums_at_bench_shapes, the mask
sum exact, the L1 sum 1e-6 relative.  The SSIM sum may be off by no more than its terms: the per-window bound of the map,
5e-6 + 1e-6 dist, summed over the windows -- at most 0.04 here (6 732 windows at 2x3x19x68), where one lost or doubled
window of a random image moves the sum by 0.1 - 0.5.
"""
import functools

import pytest
import torch

from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3, 3), (2, 3, 11, 35), (1, 2, 3, 4), (2, 3, 19, 68), (1, 3, 17, 128)]
_ids = lambda s: 'x'.join(map(str, s))  # noqa: E731


def cu(t):
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs of one shape and every oracle result the tests compare with (computed once, never modified)."""
    from oracle import ops as O
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * H + W)
    im = torch.rand(B, C, H, W, generator=gen)
    rec = torch.rand(B, C, H, W, generator=gen)
    mask = (torch.rand(B, 1, H, W, generator=gen) > 0.2).float()
    up = torch.randn(B, C, H - 2, W - 2, generator=gen)
    case = {'im': im, 'rec': rec, 'mask': mask, 'up': up}
    for key, m in (('masked', mask), ('plain', torch.ones(B, 1, H, W))):
        r = rec.clone().requires_grad_(True)
        l1 = ((im - r).abs() * m).double().sum()  # fp32 terms as the kernels form them, added without rounding
        dist = O.ssim(r * m, im * m)
        ss = dist.double().sum()
        rg, = torch.autograd.grad(0.3 * l1 + 0.7 * ss, [r])
        case[key] = {'l1': l1.detach(), 'ss': ss.detach(), 'msum': m.sum(), 'grad': rg,
                     'ss_bound': float((5e-6 + 1e-6 * dist.detach().double()).sum())}
    a, b = rec.clone().requires_grad_(True), im.clone().requires_grad_(True)
    y = O.ssim(a, b)
    ga, gb = torch.autograd.grad(y, [a, b], up)
    case['map'] = {'y': y.detach(), 'ga': ga, 'gb': gb}
    return case


@pytest.mark.parametrize('masked', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_photo_sums_off_fixture_sizes(shape, masked):
    """losses/flow_loss.py:13-27 -- photo_fwd_kernel / photo_bwd_kernel (W % 4 != 0), photo4::fwd_kernel / bwd_kernel."""
    from arflow_amd import functional as AF
    case = _case(shape)
    ref = case['masked' if masked else 'plain']
    rc = cu(case['rec']).requires_grad_(True)
    s = AF.PhotoSumsFunction.apply(cu(case['im']), rc, cu(case['mask']) if masked else None)
    assert_close(s[0], ref['l1'], 0, 1e-6, 'sum |im - rec| mask')
    assert ref['ss_bound'] <= 0.04  # far below what one lost or doubled window moves the sum by
    assert_close(s[1], ref['ss'], ref['ss_bound'], 0, 'sum SSIM distance')
    assert_close(s[2], ref['msum'], 0, 0, 'sum mask')
    gg, = torch.autograd.grad(0.3 * s[0] + 0.7 * s[1], [rc])
    rg = ref['grad']
    assert_close(gg, rg, (1e-3 * float(rg.abs().max())) / 20, 5e-5, 'd / d recons')


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_ssim_map_off_fixture_sizes(shape):
    """losses/loss_blocks.py:65-84 -- the map output of the forward kernels and the upstream-map branch of the backward."""
    from arflow_amd import loss_blocks as LB
    case = _case(shape)
    ref = case['map']
    a, b = cu(case['rec']).requires_grad_(True), cu(case['im']).requires_grad_(True)
    y = LB.SSIM(a, b)
    assert_close(y, ref['y'], 5e-6, 1e-6, 'ssim map')
    ga, gb = torch.autograd.grad(y, [a, b], cu(case['up']))
    for got, key in ((ga, 'ga'), (gb, 'gb')):
        assert_close(got, ref[key], 1e-4 * float(ref[key].abs().max()), 5e-4, 'ssim map ' + key)
