"""CPU: the float64 restatement of MseLoss (tests/mse_ref.py) against the reference's own float64 run (tests/golden/mse.npz,
tools/make_mse_golden.py), its resize against ATen's, the argument checks of the raw entry points of csrc/mse.hip, and the
Python layer's wiring (get_loss, the errors MseLoss raises, the train_step workload).  DESIGN.md section 28."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'mse.npz'), allow_pickle=False)


@pytest.mark.parametrize('tag', list(R.CASES))
def test_restatement_matches_the_reference_float64_run(gold, tag):
    """The same float64 arithmetic in another summation order: rtol 1e-12 on the four outputs, and on the gradient relative to
    its largest element (a sum of products cancels per element)."""
    inp = R.make_inputs(tag)
    for k in ('net', 'target', 'eps'):
        assert np.array_equal(inp[k], gold['%s_%s' % (k, tag)]), k  # the recipe has not drifted from the stored inputs
    r = R.mse_loss(R.case_cfg(tag), inp['net'], inp['target'], inp['eps'])
    for k in R.OUTPUTS:
        want = float(gold['%s_%s' % (k, tag)])
        assert abs(r[k] - want) <= 1e-12 * abs(want), (k, r[k], want)
    want = gold['gnet_' + tag]
    assert want.dtype == np.float64 and r['gnet'].shape == want.shape
    assert np.abs(r['gnet'] - want).max() <= 1e-12 * np.abs(want).max()
    if R.CASES[tag]['diag']:
        assert r['offdiag'] == 0 and not want[:, 4:].any()
    else:
        assert want[:, 4:6, :, -1].any() == 0 and want[:, 6:8, -1, :].any() == 0 and want[:, 4:8].any()


def test_fused_sums_restatement_agrees_with_the_loss_restatement():
    """sums() / sums_grad() (what the kernels compute) composed with the loss's coefficients give mse_loss() for the diagonal
    cases: the two restatements the GPU tests lean on say the same thing."""
    for tag in ('A', 'B'):
        cfg, inp = R.case_cfg(tag), R.make_inputs(tag)
        B, _, h, w = inp['net'].shape
        S, inv = cfg['n_samples'], cfg['inv_cov']
        full = R.mse_loss(cfg, inp['net'], inp['target'], inp['eps'])
        mode = R.MODE_INV if inv else R.MODE_COV
        f = R.sums(inp['net'], inp['target'], inp['eps'], S, mode, cfg['align_corners'])
        cm, ce = cfg['w_mse'] / (S * B * 2 * h * w), cfg['w_entropy'] / (B * h * w) * (-1 if inv else 1)
        assert abs(cm * f['sums'][0] - full['mse']) <= 1e-12 * full['mse']
        assert abs(ce * f['sums'][1] - full['entropy']) <= 1e-12 * abs(full['entropy'])
        g = R.sums_grad(inp['net'], inp['target'], inp['eps'], S, mode, cfg['align_corners'], np.array([cm, -ce, 0., 0.]))
        assert np.abs(g['gnet'] - full['gnet']).max() <= 1e-12 * np.abs(full['gnet']).max()
        assert (g['bound'][:, 0:4] > 0).all() and f['bound0'] > 0


@pytest.mark.parametrize('align', [False, True])
def test_resize_restatement_holds_atens_fp32_resize_inside_the_bound(align):
    """ATen's own fp32 bilinear resize at the GPU test's shapes lies inside the per-element bound of mse_ref.interpolate, so
    the bound the kernel is held to holds for the reference's arithmetic too; the float64 resize agrees with ATen's float64."""
    for shape in R.SHAPES:
        B, S, (h, w), (H, W) = shape
        t = torch.from_numpy(R.kernel_inputs(shape)['target'])
        ref, bound = R.interpolate(t.numpy(), (h, w), align)
        a64 = torch.nn.functional.interpolate(t.double(), (h, w), mode='bilinear', align_corners=align).numpy()
        assert np.abs(a64 - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
        a32 = torch.nn.functional.interpolate(t, (h, w), mode='bilinear', align_corners=align).double().numpy()
        err = np.abs(a32 - ref)
        print(shape, align, 'max err / bound %.3f' % float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), shape
        gt, gbound = R.resize_flow(t.numpy(), (h, w), align)
        assert np.allclose(gt[:, 0] * (W / w), ref[:, 0], rtol=1e-14, atol=0) and (gbound >= bound / max(W / w, H / h)).all()


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_check_their_arguments(lib):
    """Validation happens before any launch, so these are safe without a GPU."""
    ENULL, ESHAPE, EPARAM = -1001, -1002, -1003
    p = [ctypes.c_void_p(4096 * (i + 1) * 64) for i in range(8)]  # far apart: no overlap
    net, tgt, ez, work, sums, gsums, gnet, gz = p
    B, S, C, h, w, H, W = 2, 3, 8, 4, 6, 16, 24
    good = dict(net=net, net_bs=C * h * w, C=C, tgt=tgt, tgt_bs=2 * H * W, H=H, W=W, ez=ez, ez_bs=2 * h * w, B=B, S=S, h=h, w=w,
                mode=0, align=0, work=work, sums=sums, gsums=gsums, gnet=gnet, gnet_bs=C * h * w, gz=gz, gz_bs=2 * h * w)

    def fwd(**ch):
        a = dict(good, **ch)
        return lib.arflow_mse_fwd(a['net'], a['net_bs'], a['C'], a['tgt'], a['tgt_bs'], a['H'], a['W'], a['ez'], a['ez_bs'], a['B'],
                                  a['S'], a['h'], a['w'], a['mode'], a['align'], a['work'], a['sums'], None)

    def bwd(**ch):
        a = dict(good, **ch)
        return lib.arflow_mse_bwd(a['net'], a['net_bs'], a['C'], a['tgt'], a['tgt_bs'], a['H'], a['W'], a['ez'], a['ez_bs'],
                                  a['gsums'], a['gnet'], a['gnet_bs'], a['gz'], a['gz_bs'], a['B'], a['S'], a['h'], a['w'],
                                  a['mode'], a['align'], None)
    shared = [(dict(net=None), ENULL), (dict(tgt=None), ENULL), (dict(ez=None), ENULL),
              (dict(B=0), ESHAPE), (dict(S=0), ESHAPE), (dict(h=0), ESHAPE), (dict(W=0), ESHAPE),
              (dict(net_bs=C * h * w - 1), ESHAPE), (dict(tgt_bs=2 * H * W - 1), ESHAPE), (dict(ez_bs=2 * h * w - 1), ESHAPE),
              (dict(S=32768), ESHAPE),                       # S B = 65536 > 65535
              (dict(C=3), ESHAPE), (dict(mode=2, C=7), ESHAPE), (dict(mode=2, h=1), ESHAPE),
              (dict(mode=3), EPARAM), (dict(align=2), EPARAM)]
    for change, want in shared:
        assert fwd(**change) == want, ('fwd', change)
        assert bwd(**change) == want, ('bwd', change)
    assert fwd(work=None) == ENULL and fwd(sums=None) == ENULL
    assert bwd(gsums=None) == ENULL and bwd(gnet=None) == ENULL and bwd(mode=2, gz=None) == ENULL
    assert bwd(gnet_bs=C * h * w - 1) == ESHAPE and bwd(mode=2, gz_bs=2 * h * w - 1) == ESHAPE
    assert fwd(sums=net) == EPARAM and bwd(gnet=net) == EPARAM and bwd(mode=2, gz=ez) == EPARAM  # an output over an input
    assert lib.arflow_mse_work_size(2, 40, 52) == 4 * 9 * 2 and lib.arflow_mse_work_size(0, 4, 4) == ESHAPE
    assert lib.arflow_mse_work_size(65536, 4, 4) == ESHAPE

    def resize(**ch):
        a = dict(dict(flow=tgt, fbs=2 * H * W, out=gnet, obs=2 * h * w, B=B, align=0), **ch)
        return lib.arflow_resize_flow(a['flow'], a['fbs'], H, W, a['out'], a['obs'], a['B'], h, w, a['align'], None)
    assert resize(flow=None) == ENULL and resize(out=None) == ENULL
    assert resize(B=0) == ESHAPE and resize(B=65536) == ESHAPE and resize(fbs=2 * H * W - 1) == ESHAPE
    assert resize(obs=2 * h * w - 1) == ESHAPE and resize(align=-1) == EPARAM and resize(out=tgt) == EPARAM


def _cfg(**kw):
    from arflow_amd.config import AttrDict
    return AttrDict(dict(R.case_cfg('D'), **kw))


def test_get_loss_returns_mse_loss():
    from arflow_amd.losses import get_loss
    from arflow_amd.losses.mse_loss import MseLoss
    for tag in R.CASES:
        assert isinstance(get_loss(_cfg(**R.case_cfg(tag))), MseLoss)


def test_a_config_that_selects_no_mode_is_refused_at_construction():
    """The convention of UFlowElboLoss: NotImplementedError naming the key, where the config is first read -- not an
    AttributeError inside the first step."""
    from arflow_amd.config import AttrDict
    from arflow_amd.losses import get_loss
    with pytest.raises(NotImplementedError, match='w_mse, w_entropy, diag, inv_cov, n_samples'):
        get_loss(AttrDict(type='mse'))
    with pytest.raises(NotImplementedError, match='inv_cov'):
        get_loss(AttrDict({k: v for k, v in R.case_cfg('A').items() if k != 'inv_cov'}))
    diag_only = {k: v for k, v in R.case_cfg('A').items() if k not in ('diag_dominant', 'approx_entropy', 'offdiag_reg')}
    get_loss(AttrDict(diag_only))                                 # a diagonal mode needs none of the 4-neighbour keys
    with pytest.raises(NotImplementedError, match='diag_dominant, approx_entropy, offdiag_reg'):
        get_loss(AttrDict(dict(diag_only, diag=False)))
    for bad in (0, 1.5, True, 'two'):
        with pytest.raises(NotImplementedError, match='n_samples'):
            get_loss(_cfg(n_samples=bad))
    loss = get_loss(_cfg())
    loss.cfg.n_samples = 0                                        # the config is read on every call
    with pytest.raises(NotImplementedError, match='n_samples'):
        loss([None, None, torch.zeros(2, 8, 4, 4)], torch.zeros(2, 2, 8, 8))


def test_loss_raises_as_specified():
    from arflow_amd.losses import get_loss
    tgt = torch.zeros(2, 2, 8, 8)
    with pytest.raises(ValueError, match=r'\(2, 3, 4, 4\)'):
        get_loss(_cfg(diag=True))([None, None, torch.zeros(2, 3, 4, 4)], tgt)          # too few channels, diag
    with pytest.raises(ValueError, match=r'\(2, 7, 4, 4\)'):
        get_loss(_cfg())([None, None, torch.zeros(2, 7, 4, 4)], tgt)                   # too few channels, 4-neighbour
    with pytest.raises(ValueError, match=r'\(2, 8, 1, 4\)'):
        get_loss(_cfg())([None, None, torch.zeros(2, 8, 1, 4)], tgt)                   # h < 2 without diag
    with pytest.raises(ValueError, match=r'\(2, 8, 4, 1\)'):
        get_loss(_cfg())([None, None, torch.zeros(2, 8, 4, 1)], tgt)
    net = torch.zeros(2, 8, 4, 4)
    with pytest.raises(ValueError, match='target'):
        get_loss(_cfg())([None, None, net], torch.zeros(3, 2, 8, 8))                   # batch mismatch
    with pytest.raises(ValueError, match='target'):
        get_loss(_cfg())([None, None, net], torch.zeros(2, 3, 8, 8))                   # channel mismatch
    with pytest.raises(ValueError, match='eps'):
        get_loss(_cfg())([None, None, net], tgt, eps=torch.zeros(2, 2, 4, 4))          # n_samples = 2 needs 4 samples
    with pytest.raises(NotImplementedError, match='approx_entropy'):
        get_loss(_cfg(approx_entropy=True, n_samples=2))([None, None, net], tgt)
    from arflow_amd import _lib
    with pytest.raises(_lib.ArflowHipError):                                           # GPU only: no CPU fallback
        get_loss(_cfg(diag=True))([None, None, net], tgt, eps=torch.zeros(4, 2, 4, 4))


def test_workload_entry_is_the_shipped_config():
    from arflow_amd.config import AttrDict
    from arflow_amd.losses import get_loss
    from arflow_amd.losses.mse_loss import MseLoss
    from arflow_amd.models import get_model
    from arflow_amd.train_step import WORKLOADS
    mcfg, lcfg = WORKLOADS['pwcprobflow+mse_loss']
    assert lcfg == dict(type='mse', w_mse=1.0, w_entropy=0.1, diag=False, diag_dominant=False, inv_cov=True,
                        approx_entropy=False, offdiag_reg=1000.0, n_samples=1)      # configs/chairs_uflow_mse.json:8-16
    assert mcfg == dict(type='uflow_prob', feature_norm=True, level_dropout=0.1, out_channels=[2, 2, 4], inv_cov=True,
                        n_pyramids=1, mixture_weights=False)
    assert isinstance(get_loss(AttrDict(lcfg)), MseLoss)
    model = get_model(AttrDict(mcfg))
    assert sum(p.numel() for p in model.parameters()) > 0
