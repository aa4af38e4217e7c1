"""The CPU oracle against the REFERENCE's own pure-PyTorch functions on a seeded random sweep -- on top of the analytic
and ragged cases of tests/test_oracle_golden.py.  The reference's outputs and autograd gradients of the sweep are frozen
in tests/golden/reference_sweep.npz (oracle/make_golden.py --only sweep, which runs the reference); the inputs are
regenerated here from their seeds and checked against stored fingerprints, and the oracle is run on them live.
Correlation and warp results are stored as exact residuals from a float64 prediction (oracle/fixture_common.py)."""
import pytest
import torch

from oracle.fixture_common import (fingerprint, predict_corr, predict_flow_warp, residual_decode, sweep_corr_inputs,
                                   sweep_mask_inputs, sweep_warp_inputs)


@pytest.fixture(scope='module')
def ref(golden):
    return golden('reference_sweep')


def _check_inputs(ref, prefix, **tensors):
    for name, t in tensors.items():
        assert torch.equal(fingerprint(t), ref['%s_fp_%s' % (prefix, name)]), \
            '%s: seeded input %s differs from the one the fixture was made from' % (prefix, name)


def _reference(ref, key, pred):
    """The reference's fp32 result `key`, rebuilt bit-exactly from its residual against `pred`."""
    y = residual_decode(ref[key + '_r'], pred)
    want = float(ref[key + '_sum'])
    assert abs(float(y.double().sum()) - want) <= 1e-9 * float(y.double().abs().sum()) + 1e-12, key + ': residual decode'
    return y


def _close(a, b, atol, rtol, what):
    err = (a.double() - b.double()).abs()
    assert bool((err <= atol + rtol * b.double().abs()).all()), '%s: max err %.3e' % (what, float(err.max()))


@pytest.mark.parametrize('shape', [(2, 32, 24, 40), (1, 7, 9, 33), (3, 16, 8, 14)])
def test_correlation_live(ref, shape):
    from oracle import ops as O
    tag = 'corr_%s' % 'x'.join(str(s) for s in shape)
    x1, x2, go = sweep_corr_inputs(shape)
    _check_inputs(ref, tag, x1=x1, x2=x2, g=go)
    y_ref, r1, r2 = (_reference(ref, tag + k, p) for k, p in zip(('_y', '_gx1', '_gx2'), predict_corr(x1, x2)(go)))
    _close(O.correlation(x1, x2, 4), y_ref, 1e-6, 1e-5, 'corr fwd')  # models/correlation_native.py:13-23
    o1, o2 = O.correlation_backward(go, x1, x2, 4)
    _close(o1, r1, 5e-6, 1e-5, 'corr gx1')
    _close(o2, r2, 5e-6, 1e-5, 'corr gx2')


@pytest.mark.parametrize('pad', ['zeros', 'border'])
@pytest.mark.parametrize('ac', [True, False])
def test_flow_warp_live(ref, pad, ac):
    from oracle import ops as O
    x, fl, go = sweep_warp_inputs()
    _check_inputs(ref, 'warp', x=x, flow=fl, g=go)
    a, f = x.clone().requires_grad_(True), fl.clone().requires_grad_(True)
    y = O.flow_warp(a, f, pad=pad, align_corners=ac)  # utils/warp_utils.py:83-90
    got = (y,) + torch.autograd.grad(y, [a, f], go)
    tag = 'warp_%s_%d' % (pad, int(ac))
    for a, n, p in zip(got, ('y', 'gsrc', 'gflow'), predict_flow_warp(x, fl, pad, ac)(go)):
        _close(a, _reference(ref, '%s_%s' % (tag, n), p), 2e-5, 1e-4, 'flow_warp ' + n)


def test_masks_and_losses_live(ref):
    from oracle import ops as O
    fl, im1, im2, mask = sweep_mask_inputs()
    _check_inputs(ref, 'm', flow=fl, im1=im1, im2=im2, mask=mask)
    _close(O.compute_range_map(fl), ref['m_range_map'], 1e-6, 1e-5, 'range map')  # uflow_utils.py:80-160
    _close(O.border_mask(fl), ref['m_border_mask'], 0, 0, 'border mask')          # warp_utils.py:119-134
    _close(O.mask_invalid(O.flow_to_warp(fl)), ref['m_mask_invalid'], 0, 0, 'mask_invalid')
    for ps in (7, 3):
        b = im2.clone().requires_grad_(True)
        y = O.census_loss(im1, b, mask, ps)  # utils/uflow_utils.py:282-293
        gb, = torch.autograd.grad(y, [b])
        _close(y, ref['m_census%d' % ps], 1e-6, 1e-5, 'census loss')
        _close(gb, ref['m_census%d_g' % ps], 1e-7, 1e-4, 'census grad')
    _close(O.ssim(im1, im2), ref['m_ssim'], 5e-6, 1e-5, 'ssim')                    # loss_blocks.py:65-84
    _close(O.smooth_grad_1st(fl, im1, 10.), ref['m_smooth1'], 1e-7, 1e-5, 'smooth 1st')
    _close(O.smooth_grad_2nd(fl, im1, 10.), ref['m_smooth2'], 1e-7, 1e-5, 'smooth 2nd')
