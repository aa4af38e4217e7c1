"""CPU: the float64 restatement of the augmentation-regularisation arithmetic (tests/ar_ref.py) against the reference's own
flow_warp, border_mask and abs_robust_loss where a checkout is at hand (ARFLOW_REFERENCE), the mutations that show the derived
bounds and the GPU tests' cap hide nothing, draw_ar_params, theta_from_augment, the argument checks of the raw entry points of
csrc/ar.hip and the host refusals of arflow_amd/ar.py.  DESIGN.md section 41.

The comparison against the reference uses a theta with NO s within 1e-3 of 0, W - 1 or H - 1 (checked below), so that the
float32 reference has no mask decision it could take the other way.  The non-strict-border mutation can only show where some
s lies EXACTLY on the border, so it alone runs on the whole-pixel variant of the same inputs (ar_ref.case(integer_shift=True):
the third sample's translation in whole pixels, s computed without rounding, a column and a row of it on the border); every
other mutation runs on the inputs of the comparison."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from arflow_amd import ar as AR
from arflow_amd import augment as A
from tests import ar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [((37, 53), 6), ((40, 64), 1)]
# Largest |restatement - reference composition| measured on the CPU over SIZES (the reference's float32 grid_sample and
# border_mask, the 2 x 2 product in float64, against the float64 restatement): img 4.98e-6, flow 3.97e-5, mask 1.14e-6.  It is
# grid_sample's normalise / un-normalise round trip (2 s / (W - 1) - 1 and back: a few u W of s, times the neighbour
# differences of the plane, up to ~ 15 for this flow), which the kernel does not make, and grid_sample's own fp32 blend.  The
# loss: 1.9e-9 relative on the value and 1.4e-7 of the largest gradient, both the rounding of eps = 0.01 and q = 0.4 to the
# float32 numbers the kernels receive (0 at eps = 0, q = 1).  The tolerances are 4 x the measured values.
TOL_IMG, TOL_FLOW, TOL_MASK, TOL_LOSS, TOL_GRAD = 4 * 4.98e-6, 4 * 3.97e-5, 4 * 1.14e-6, 4 * 1.9e-9, 4 * 1.4e-7


def _reference(rel, name):
    root = os.environ.get('ARFLOW_REFERENCE')
    path = os.path.join(root, *rel) if root else None
    if not path or not os.path.exists(path):
        pytest.skip('no checkout of the reference (ARFLOW_REFERENCE)')
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _displacement(theta, hw):
    """d = s - p' in float32, from s in float64: what a caller hands the reference's flow_warp."""
    H, W = hw
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    th = theta.double()
    a, b, tx, c, d, ty = (th[:, k].reshape(-1, 1, 1) for k in range(6))
    return torch.stack([a * xs + b * ys + tx - xs, c * xs + d * ys + ty - ys], 1).float()


@pytest.mark.parametrize('hw,C', SIZES, ids=['37x53', '40x64'])
def test_restatement_matches_the_reference_functions(hw, C):
    W = _reference(('utils', 'warp_utils.py'), '_ref_warp_utils')
    theta, img, flow, noc = R.case(hw, C)
    r = R.transform(theta, img, flow, noc)
    margin = R.border_margin(r['s'], hw)
    assert margin > 1e-3, margin   # no mask decision the float32 reference could legitimately take the other way
    d = _displacement(theta, hw)
    th = theta.double()
    a, b, c, dd = (th[:, k].reshape(-1, 1, 1) for k in (0, 1, 3, 4))
    img_t = W.flow_warp(img, d, pad='zeros', align_corners=True)
    g = W.flow_warp(flow, d, pad='zeros').double()
    det = a * dd - b * c
    flow_t = torch.stack([(dd * g[:, 0] - b * g[:, 1]) / det, (-c * g[:, 0] + a * g[:, 1]) / det], 1)
    mask_t = W.flow_warp(noc, d, pad='zeros') * W.border_mask(d)
    errs = [float((x.double() - y).abs().max()) for x, y in ((img_t, r['img_t']), (flow_t, r['flow_t']), (mask_t, r['mask_t']))]
    print('%dx%d margin %.3e: |reference - restatement| img %.3e flow %.3e mask %.3e' % (hw + (margin,) + tuple(errs)))
    assert errs[0] <= TOL_IMG and errs[1] <= TOL_FLOW and errs[2] <= TOL_MASK, errs
    ones = R.transform(theta, noc=None, flow=flow)['mask_t']
    assert float((ones - (W.flow_warp(torch.ones_like(noc), d, pad='zeros') * W.border_mask(d)).double()).abs().max()) <= TOL_MASK


@pytest.mark.parametrize('eps,q', [(0.0, 1.0), (0.01, 0.4)])
def test_loss_restatement_matches_abs_robust_loss(eps, q):
    P = _reference(('losses', 'penalty_functions.py'), '_ref_penalty_functions')
    pred, flow_t, m = R.loss_case()
    for mask in (None, m):
        p = pred.double().requires_grad_(True)
        mm = torch.ones_like(m).double() if mask is None else mask.double()
        want = (P.abs_robust_loss(p - flow_t.double(), eps=eps, q=q) * mm).mean() / (mm.mean() + 1e-7)
        want.backward()
        value, grad = R.loss(pred, flow_t, mask, eps, q)
        assert abs(float(value - want.detach())) <= TOL_LOSS * abs(float(want.detach()))
        assert float((grad - p.grad).abs().max()) <= TOL_GRAD * float(p.grad.abs().max())   # sign(0) = 0 on both sides


@pytest.mark.parametrize('hw,C', SIZES, ids=['37x53', '40x64'])
def test_every_mutation_exceeds_the_derived_bound(hw, C):
    cap = R.mutation_cap(hw, C)
    for mut in R.MUTATIONS:
        args = R.case(hw, C, integer_shift=(mut == 'nonstrict'))
        good, bad = R.transform(*args, track=True), R.transform(*args, mutate=mut)
        caught = 0
        for k, e in (('img_t', 'e_img'), ('flow_t', 'e_flow'), ('mask_t', 'e_mask')):
            assert torch.isfinite(good[e]).all() and float(good[e].max()) <= cap, (mut, k, float(good[e].max()), cap)
            caught += int(((good[k] - bad[k]).abs() > good[e]).sum())
        print('%dx%d %-9s caught at %d values (cap %.3f)' % (hw + (mut, caught, cap)))
        assert caught > 0, mut


def test_anchors_are_exact_in_the_restatement():
    """Identity, flip and whole-pixel translation: bound 0 everywhere, and the values are the inputs' own."""
    hw = (9, 12)
    g = torch.Generator().manual_seed(3)
    img, flow, noc = torch.rand(2, 3, *hw, generator=g), torch.randn(2, 2, *hw, generator=g), torch.rand(2, 1, *hw, generator=g)
    theta = torch.tensor([[1, 0, 0, 0, 1, 0], [-1, 0, hw[1] - 1, 0, 1, 0]], dtype=torch.float32)
    r = R.transform(theta, img, flow, noc, track=True)
    assert float(r['e_img'].max()) == 0 and float(r['e_flow'].max()) == 0 and float(r['e_mask'].max()) == 0
    border = torch.zeros(1, *hw, dtype=torch.float64)
    border[:, 1:-1, 1:-1] = 1
    assert torch.equal(r['img_t'][0], img[0].double()) and torch.equal(r['img_t'][1], img[1].flip(-1).double())
    assert torch.equal(r['flow_t'][1, 0], -flow[1, 0].flip(-1).double()) and torch.equal(r['flow_t'][1, 1], flow[1, 1].flip(-1).double())
    assert torch.equal(r['mask_t'][0], noc[0].double() * border) and torch.equal(r['mask_t'][1], noc[1].flip(-1).double() * border)


# ---- draw_ar_params, theta_from_augment -----------------------------------------------------------------------------------
def test_draw_ar_params_identity_when_nothing_is_configured():
    g = torch.Generator().manual_seed(0)
    state = g.get_state()
    for cfg in (None, {}, dict(zoom=None, rotate=0, trans=0.0, hflip=False)):
        t = AR.draw_ar_params(cfg, 5, (37, 53), g)
        assert t.dtype == torch.float32 and torch.equal(t, AR.identity_theta(5))
    assert torch.equal(g.get_state(), state)   # only what is configured is drawn


def test_draw_ar_params_ranges_seed_and_determinant():
    H, W, n = 48, 80, 1000
    cfg = dict(zoom=(0.8, 1.5), rotate=0.2, trans=0.1, hflip=True)
    t = AR.draw_ar_params(cfg, n, (H, W), torch.Generator().manual_seed(4))
    again = AR.draw_ar_params(cfg, n, (H, W), torch.Generator().manual_seed(4))
    other = AR.draw_ar_params(cfg, n, (H, W), torch.Generator().manual_seed(5))
    assert torch.equal(t, again) and not torch.equal(t, other) and tuple(t.shape) == (n, 6)
    a, b, tx, c, d, ty = (t[:, k].double() for k in range(6))
    det = a * d - b * c
    assert float(det.abs().min()) > 0
    z = det.abs().rsqrt()                                   # det = +-1 / z^2
    assert 0.8 - 1e-6 <= float(z.min()) and float(z.max()) <= 1.5 + 1e-6 and float(z.min()) < 0.81 and float(z.max()) > 1.49
    flipped = det < 0
    assert 0.45 < float(flipped.double().mean()) < 0.55
    phi = torch.atan2(-b, d)                                # b = -sin / z, d = cos / z
    assert float(phi.abs().max()) <= 0.2 + 1e-6 and float(phi.min()) < -0.19 and float(phi.max()) > 0.19
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    taux, tauy = tx - (cx - (a * cx + b * cy)), ty - (cy - (c * cx + d * cy))
    assert float(taux.abs().max()) <= 0.1 * W + 1e-4 and float(tauy.abs().max()) <= 0.1 * H + 1e-4
    assert float(taux.abs().max()) > 0.099 * W and float(tauy.abs().max()) > 0.099 * H
    only = AR.draw_ar_params(dict(hflip=True), 64, (H, W), torch.Generator().manual_seed(1))
    assert set(only[:, 0].tolist()) == {1.0, -1.0} and set(only[:, 2].tolist()) == {0.0, float(W - 1)}
    with pytest.raises(ValueError, match='zoom'):
        AR.draw_ar_params(dict(zoom=(0.0, 1.0)), 2, (H, W), torch.Generator())


def test_theta_from_augment_against_make_params():
    p = A.make_params((13, 22), (7, 10), [0, 6, 3], [12, 0, 5], flip=[False, True, True])
    t = AR.theta_from_augment(p)
    assert t.tolist() == [[1, 0, 12, 0, 1, 0], [-1, 0, 9, 0, 1, 6], [-1, 0, 14, 0, 1, 3]]
    gt = torch.randn(3, 2, 13, 22, generator=torch.Generator().manual_seed(2))
    r = R.transform(t, flow=gt, out_hw=p.out_hw, track=True)
    want = torch.stack([gt[0, :, 0:7, 12:22], gt[1, :, 6:13, 0:10].flip(-1), gt[2, :, 3:10, 5:15].flip(-1)]).double()
    want[1:, 0] = -want[1:, 0]
    assert torch.equal(r['flow_t'], want) and float(r['e_flow'].max()) == 0
    # with the resize: the centre of output pixel x' is crop coordinate (x' + 1/2) tw / w - 1/2, as F.interpolate places it
    p = A.make_params((13, 22), (7, 10), [2], [4], flip=[False], scale_hw=(14, 20))
    t = AR.theta_from_augment(p)
    assert t.tolist() == [[0.5, 0, 4 - 0.25, 0, 0.5, 2 - 0.25]]
    ramp = torch.arange(22, dtype=torch.float32).reshape(1, 1, 1, 22).expand(1, 3, 13, 22).contiguous()
    got = R.transform(t, img=ramp, out_hw=(14, 20))['img_t']
    want = torch.nn.functional.interpolate(ramp[:, :, 2:9, 4:14].double(), (14, 20), mode='bilinear', align_corners=False)
    assert float((got - want)[..., 1:-1].abs().max()) <= 1e-12   # all but the first and last column, which the resize clamps
    with pytest.raises(ValueError, match='AugmentParams'):
        AR.theta_from_augment(t)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


NAMES = ('arflow_ar_transform', 'arflow_ar_loss_partials', 'arflow_ar_loss_fwd', 'arflow_ar_loss_bwd')


def test_symbols_are_declared_exported_and_bound(lib):
    from arflow_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'arflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert m, name
        assert hasattr(raw, name) and name in _lib.PROTOTYPES
        assert len([p for p in m.group(1).split(',') if p.strip()]) == len(_lib.PROTOTYPES[name]), name
    assert lib.arflow_abi_version() == 10 and _lib.ABI_VERSION == 10


def test_entry_points_check_their_arguments(lib):
    """Validation happens before any launch, so these are safe without a GPU."""
    ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
    ptr = [ctypes.c_void_p(4096 * (i + 1) * 64) for i in range(8)]
    good = dict(theta=ptr[0], img=ptr[1], img_t=ptr[2], C=6, flow=ptr[3], flow_t=ptr[4], noc=ptr[5], mask_t=ptr[6], B=3, Hs=37, Ws=53,
                H=37, W=53)

    def transform(**ch):
        a = dict(good, **ch)
        return lib.arflow_ar_transform(a['theta'], a['img'], a['img_t'], a['C'], a['flow'], a['flow_t'], a['noc'], a['mask_t'], a['B'],
                                       a['Hs'], a['Ws'], a['H'], a['W'], None)
    for change, want in [(dict(theta=None), ENULL), (dict(img=None), ENULL), (dict(flow=None), ENULL),
                         (dict(img_t=None, flow_t=None, mask_t=None), EPARAM),
                         (dict(B=0), ESHAPE), (dict(B=65536), ESHAPE), (dict(H=0), ESHAPE), (dict(W=-1), ESHAPE), (dict(Hs=0), ESHAPE),
                         (dict(Ws=0), ESHAPE), (dict(C=0), ESHAPE), (dict(H=1 << 15, W=1 << 15), ESHAPE),
                         (dict(Hs=1, Ws=(1 << 24) + 1), ESHAPE)]:
        assert transform(**change) == want, change
    lgood = dict(pred=ptr[0], flow_t=ptr[1], mask=ptr[2], work=ptr[3], sums=ptr[4], gsums=ptr[5], gpred=ptr[6], B=3, H=37, W=53, eps=0.01,
                 q=0.4)

    def fwd(**ch):
        a = dict(lgood, **ch)
        return lib.arflow_ar_loss_fwd(a['pred'], a['flow_t'], a['mask'], a['work'], a['sums'], a['B'], a['H'], a['W'], a['eps'], a['q'], None)

    def bwd(**ch):
        a = dict(lgood, **ch)
        return lib.arflow_ar_loss_bwd(a['pred'], a['flow_t'], a['mask'], a['gsums'], a['gpred'], a['B'], a['H'], a['W'], a['eps'], a['q'],
                                      None)
    shared = [(dict(pred=None), ENULL), (dict(flow_t=None), ENULL), (dict(B=0), ESHAPE), (dict(H=0), ESHAPE), (dict(W=0), ESHAPE),
              (dict(H=1 << 15, W=1 << 15), ESHAPE), (dict(eps=-1.0), EPARAM), (dict(q=0.0), EPARAM), (dict(q=-1.0), EPARAM),
              (dict(q=float('nan')), EPARAM), (dict(eps=float('inf')), EPARAM), (dict(eps=0.0, q=0.4), EPARAM)]
    for change, want in shared:
        assert fwd(**change) == want, ('fwd', change)
        assert bwd(**change) == want, ('bwd', change)
    assert fwd(work=None) == ENULL and fwd(sums=None) == ENULL and bwd(gsums=None) == ENULL and bwd(gpred=None) == ENULL
    for B, H, W in ((3, 37, 53), (1, 1, 1), (8, 384, 640), (2, 64, 128), (5, 1, 2049)):
        assert lib.arflow_ar_loss_partials(B, H, W) == B * -(-(H * W) // 2048), (B, H, W)
    assert lib.arflow_ar_loss_partials(3, 37, 53) == 3 and lib.arflow_ar_loss_partials(3, 50, 53) == 6
    assert lib.arflow_ar_loss_partials(0, 4, 4) == ESHAPE and lib.arflow_ar_loss_partials(1, 4, -1) == ESHAPE
    assert lib.arflow_ar_loss_partials(1, 1 << 15, 1 << 15) == ESHAPE


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_host_refusals():
    from arflow_amd import _lib
    theta, img, flow, noc = R.case((9, 12), 3)
    with pytest.raises(_lib.ArflowHipError):
        AR.ar_transform(theta, img=img, flow=flow, noc=noc)
    with pytest.raises(_lib.ArflowHipError):
        AR.ar_loss(flow, flow)
    singular = theta.clone()
    singular[1] = torch.tensor([1.0, 2.0, 0.0, 2.0, 4.0, 0.0])
    with pytest.raises(ValueError, match='singular'):
        AR.ar_transform(singular, img=img)
    with pytest.raises(ValueError, match='theta'):
        AR.ar_transform(theta[:2], img=img)
    with pytest.raises(ValueError, match='at least one'):
        AR.ar_transform(theta)
    with pytest.raises(ValueError, match='eps > 0'):
        AR.ar_loss(flow, flow, eps=0.0, q=0.4)
    with pytest.raises(ValueError, match='eps >= 0'):
        AR.ar_loss(flow, flow, eps=-1.0)
    from arflow_amd.train_step import TrainStep
    for workload, kind in (('pwcprobflow+uflow_elbo_loss', 'uflow_elbo'), ('pwcliteprob+elbo_loss', 'elbo'), ('pwcprobflow+mse_loss', 'mse')):
        with pytest.raises(ValueError, match="loss type '%s'" % kind):
            TrainStep(workload, torch.device('cpu'), ar_cfg=dict(w_ar=0.01))
