"""GPU: the augmentation-regularisation kernels (csrc/ar.hip; arflow_amd.ar) -- anchors that are exact, every output value
against the float64 restatement of tests/ar_ref.py within the bound it derives from the inputs alone, the loss node's value,
gradient and bitwise reproducibility, and TrainStep(ar_cfg=...).  DESIGN.md section 41.

No derived bound may exceed the cap the mutations of tests/test_ar_cpu.py establish (ar_ref.mutation_cap: half the smallest
error any of the five wrong restatements makes on these inputs, computed here, not typed in).  Each test prints its largest
error / bound ratio.
Shapes: 37 x 53 with C = 6 (scalar stores, a ragged last quad) and 40 x 64 with C = 1 (float4 stores), B = 3 with three
different theta; the loss at 37 x 53 (one workgroup per sample) and 50 x 53 (two, the second ragged)."""
import contextlib

import pytest
import torch

from arflow_amd import ar as AR
from arflow_amd import augment as A
from tests import ar_ref as R

pytestmark = pytest.mark.gpu
SIZES = [((37, 53), 6), ((40, 64), 1)]
_cache = {}


def reference(hw, C):
    """Inputs, float64 references and bounds of one case, computed once and left unchanged."""
    if (hw, C) not in _cache:
        theta, img, flow, noc = R.case(hw, C)
        full = R.transform(theta, img, flow, noc, track=True)
        ones = R.transform(theta, flow=flow, track=True)
        cap = R.mutation_cap(hw, C)
        for r in (full, ones):
            for e in ('e_img', 'e_flow', 'e_mask'):
                assert r[e] is None or (torch.isfinite(r[e]).all() and float(r[e].max()) <= cap), (e, cap)
        _cache[(hw, C)] = dict(theta=theta, img=img, flow=flow, noc=noc, full=full, ones=ones, cap=cap)
    return _cache[(hw, C)]


def excess(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print('%s: max err %.3e, max bound %.3e, max err / bound %.3f' % (name, float(err.max()), float(bound.max()), ratio))
    return int((err > bound).sum())


def border(hw):
    m = torch.zeros(1, 1, *hw)
    m[:, :, 1:-1, 1:-1] = 1
    return m.cuda()


# ---- exact anchors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw,C', SIZES, ids=['37x53', '40x64'])
def test_identity_and_flip_are_exact(hw, C):
    _, img, flow, noc = (t.cuda() for t in R.case(hw, C))
    W = hw[1]
    img_t, flow_t, mask_t = AR.ar_transform(AR.identity_theta(3), img, flow, noc)
    assert torch.equal(img_t, img) and torch.equal(flow_t, flow) and torch.equal(mask_t, noc * border(hw))
    flip = torch.tensor([[-1.0, 0, W - 1, 0, 1, 0]]).repeat(3, 1)
    img_t, flow_t, mask_t = AR.ar_transform(flip.cuda(), img, flow, noc)   # theta may live on the device
    assert torch.equal(img_t, img.flip(-1))
    assert torch.equal(flow_t[:, 0], -flow[:, 0].flip(-1)) and torch.equal(flow_t[:, 1], flow[:, 1].flip(-1))
    assert torch.equal(mask_t, noc.flip(-1) * border(hw))
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (img_t, flow_t, mask_t))


@pytest.mark.parametrize('hw,C', SIZES, ids=['37x53', '40x64'])
def test_integer_translation_is_the_shifted_window(hw, C):
    _, img, flow, noc = (t.cuda() for t in R.case(hw, C))
    H, W = hw
    dx, dy = 3, -2                                             # s = (x' + 3, y' - 2)
    theta = torch.tensor([[1.0, 0, dx, 0, 1, dy]]).repeat(3, 1)
    img_t, flow_t, mask_t = AR.ar_transform(theta, img, flow, noc)

    def shifted(t):
        out = torch.zeros_like(t)
        out[:, :, -dy:, :W - dx] = t[:, :, :H + dy, dx:]
        return out
    assert torch.equal(img_t, shifted(img)) and torch.equal(flow_t, shifted(flow))
    assert float(img_t[:, :, :-dy].abs().max()) == 0 and float(img_t[:, :, :, W - dx:].abs().max()) == 0   # zeros outside
    assert torch.equal(mask_t, shifted(noc * border(hw)))      # 0 outside AND where s lies on the source's strict border
    assert float(mask_t[:, :, -dy].abs().max()) == 0 and float(mask_t[:, :, :, W - dx - 1].abs().max()) == 0
    assert float(mask_t[:, :, -dy + 1, 0].min()) > 0           # s_x = 3 at x' = 0: inside


def test_ground_truth_follows_a_crop_and_flip():
    p = A.make_params((13, 22), (7, 10), [0, 6, 3], [12, 0, 5], flip=[False, True, True])
    gt = torch.randn(3, 2, 13, 22, generator=torch.Generator().manual_seed(2)).cuda()
    _, got, mask = AR.ar_transform(AR.theta_from_augment(p), flow=gt, out_hw=p.out_hw, mask=False)
    want = torch.stack([gt[0, :, 0:7, 12:22], gt[1, :, 6:13, 0:10].flip(-1), gt[2, :, 3:10, 5:15].flip(-1)])
    want[1:, 0] = -want[1:, 0]
    assert mask is None and tuple(got.shape) == (3, 2, 7, 10) and torch.equal(got, want)
    src = torch.rand(3, 2, 3, 13, 22, generator=torch.Generator().manual_seed(3)).cuda()
    img, _ = A.augment_batch(src, p)                           # the images the ground truth now belongs to
    img_t, _, _ = AR.ar_transform(AR.theta_from_augment(p), img=src.reshape(3, 6, 13, 22), out_hw=p.out_hw)
    assert torch.equal(img_t, img)


# ---- against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw,C', SIZES, ids=['37x53-scalar', '40x64-float4'])
def test_every_value_within_its_derived_bound(hw, C):
    c = reference(hw, C)
    theta, img, flow, noc = c['theta'], c['img'].cuda(), c['flow'].cuda(), c['noc'].cuda()
    full, ones = c['full'], c['ones']
    tag = '%dx%d ' % hw
    img_t, flow_t, mask_t = AR.ar_transform(theta, img, flow, noc)
    assert float((img_t == 0).float().mean()) > 0.05           # zoom 0.8: the zero padding shows
    bad = excess(tag + 'img_t', img_t, full['img_t'], full['e_img']) + excess(tag + 'flow_t', flow_t, full['flow_t'], full['e_flow']) \
        + excess(tag + 'mask_t', mask_t, full['mask_t'], full['e_mask'])
    # each group alone, the other pointers null: the same bits
    only_img = AR.ar_transform(theta, img=img)
    only_flow = AR.ar_transform(theta, flow=flow, mask=False)
    only_mask = AR.ar_transform(theta, noc=noc)
    assert only_img[1] is None and only_img[2] is None and torch.equal(only_img[0], img_t)
    assert only_flow[0] is None and only_flow[2] is None and torch.equal(only_flow[1], flow_t)
    assert only_mask[0] is None and only_mask[1] is None and torch.equal(only_mask[2], mask_t)
    # an absent noc reads as ones
    _, f1, m1 = AR.ar_transform(theta, flow=flow)
    assert torch.equal(f1, flow_t)
    bad += excess(tag + 'mask_t of ones', m1, ones['mask_t'], ones['e_mask'])
    assert bad == 0
    print(tag + 'cap %.3f' % c['cap'])


# ---- the loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(37, 53), (50, 53)], ids=['37x53-1wg', '50x53-2wg'])
@pytest.mark.parametrize('eps,q', [(0.0, 1.0), (0.01, 0.4)])
def test_loss_value_and_gradient(hw, eps, q):
    from arflow_amd import functional as AF
    from arflow_amd import _lib
    pred, flow_t, m = R.loss_case(hw)
    assert _lib.load().arflow_ar_loss_partials(3, *hw) == (3 if hw == (37, 53) else 6) and (hw[0] * hw[1]) % 256 != 0
    same = (pred == flow_t)
    assert bool(same.any()) and not bool(same.all())
    for name, mask in (('no mask', None), ('fractional', m), ('all zero', torch.zeros_like(m))):
        value, grad, e_value, e_grad = R.loss(pred, flow_t, mask, eps, q, track=True)
        runs = []
        for det in (False, False, True):
            p = pred.cuda().requires_grad_(True)
            with AF.deterministic(det):
                out = AR.ar_loss(p, flow_t.cuda(), None if mask is None else mask.cuda(), eps=eps, q=q)
                out.backward()
            runs.append((out.detach(), p.grad))
        assert out.dtype == torch.float64 and out.dim() == 0
        for o, g in runs[1:]:                                  # two calls, and one in deterministic mode: the same bits
            assert torch.equal(o, runs[0][0]) and torch.equal(g, runs[0][1])
        out, g = runs[0]
        tag = '%dx%d eps %g q %g %s ' % (hw + (eps, q, name))
        print(tag + 'loss %.9f (float64 %.9f), |diff| %.3e, bound %.3e' % (float(out), float(value), abs(float(out) - float(value)),
                                                                           float(e_value)))
        assert abs(float(out) - float(value)) <= float(e_value)
        assert excess(tag + 'gradient', g, grad, e_grad) == 0
        if name == 'all zero':
            assert float(out) == 0 and float(g.abs().max()) == 0
        else:
            assert float(out) > 0.1 and float(g.abs().max()) > 0
        if q == 1.0:
            assert float(g[same.cuda()].abs().max()) == 0      # sign(0) = 0
    with pytest.raises(NotImplementedError, match='flow_t'):
        AR.ar_loss(pred.cuda(), flow_t.cuda().requires_grad_(True), eps=eps, q=q).backward()
    with pytest.raises(NotImplementedError, match='mask'):
        AR.ar_loss(pred.cuda().requires_grad_(True), flow_t.cuda(), m.cuda().requires_grad_(True), eps=eps, q=q).backward()


# ---- TrainStep ----------------------------------------------------------------------------------------------------------------
# The smallest input the workload itself admits: unFlowLoss weights the 1/32 scale, whose 3 x 3 SSIM window needs 3 rows and
# columns, and the pyramid wants multiples of 64.  (At 64 x 128 the step without ar_cfg already stops in arflow_photo_fwd.)
STEP_HW = (128, 128)


def _step(ar_cfg, seed=11):
    from arflow_amd.train_step import TrainStep
    kw = {} if ar_cfg is None else dict(ar_cfg=ar_cfg)
    return TrainStep('pwclite+unflow_loss', torch.device('cuda'), seed=seed, **kw)


def _ran(rec):
    return sorted({name for name, _ in rec})


AR_CALLS = ['arflow_ar_loss_bwd', 'arflow_ar_loss_fwd', 'arflow_ar_transform']


def test_train_step_with_the_ar_pass():
    """Two steps at batch 2, 128 x 128: finite loss, changed parameters, the three entry points in the call log (none of them
    without ar_cfg: test_w_ar_zero_is_the_plain_step reads the plain step's log)."""
    from arflow_amd import functional as AF
    from arflow_amd.train_step import synthetic_pairs
    x = synthetic_pairs(2, *STEP_HW, device=torch.device('cuda'), seed=5)
    step = _step(dict(w_ar=0.01, ar_eps=0.01, ar_q=0.4, mask_st=True, st_cfg=AR.DEFAULT_ST_CFG))
    before = [p.detach().clone() for p in step.model.parameters()]
    AF.start_kernel_timing()
    losses = [step(x), step(x)]
    ran = _ran(AF.stop_kernel_timing())
    assert all(bool(torch.isfinite(l)) for l in losses) and bool(torch.isfinite(step.last_ar)) and float(step.last_ar) > 0
    assert sum(not torch.equal(a, b) for a, b in zip(before, step.model.parameters())) > len(before) // 2
    assert all(bool(torch.isfinite(p).all()) for p in step.model.parameters())
    assert [n for n in ran if n.startswith('arflow_ar_')] == AR_CALLS, ran


@contextlib.contextmanager
def reproducible():
    """The setting in which two TrainSteps from one seed are bitwise equal (tools/determinism_probe.py):
    the library's deterministic mode, and the vendor library held to its deterministic convolution solvers."""
    from arflow_amd import functional as AF
    saved = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        with AF.deterministic():
            yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved


def test_w_ar_zero_is_the_plain_step():
    """With w_ar = 0 the step is the plain step BIT FOR BIT, loss and every parameter after it: the second pass runs, its loss
    is multiplied by 0.0, so every gradient it sends back is +-0 and the sum of the two losses is the first.  Run-to-run
    equality of a train step is torch.equal in the reproducible setting (tests/test_augment_gpu.py compares losses so, DESIGN.md
    section 14 records it for the parameter gradients of this workload); two plain steps are compared first to show it holds
    at this size.  The plain step's call log holds no entry point of ar.py, the w_ar = 0 step's all three."""
    from arflow_amd import functional as AF
    from arflow_amd.train_step import synthetic_pairs
    x = synthetic_pairs(2, *STEP_HW, device=torch.device('cuda'), seed=5)
    params, losses, logs = [], [], []
    with reproducible():
        for cfg in (None, None, dict(w_ar=0.0, ar_eps=0.01, ar_q=0.4, st_cfg=AR.DEFAULT_ST_CFG)):
            step = _step(cfg)
            AF.start_kernel_timing()
            losses.append(step(x))
            logs.append(_ran(AF.stop_kernel_timing()))
            params.append([p.detach().clone() for p in step.model.parameters()])
            assert (step.last_ar is None) == (cfg is None)
    assert len(logs[0]) > 5 and not [n for n in logs[0] if n.startswith('arflow_ar_')], logs[0]
    assert [n for n in logs[2] if n.startswith('arflow_ar_')] == AR_CALLS, logs[2]
    assert bool(torch.isfinite(step.last_ar)) and float(step.last_ar) > 0      # the second pass ran
    flat = [torch.cat([p.reshape(-1) for p in ps]) for ps in params]
    print('largest |difference| of the parameters: plain run to run %.3e, w_ar = 0 against plain %.3e; losses %.9f %.9f %.9f'
          % (float((flat[0] - flat[1]).abs().max()), float((flat[2] - flat[0]).abs().max()), float(losses[0]), float(losses[1]),
             float(losses[2])))
    assert torch.equal(losses[0], losses[1]) and all(torch.equal(a, b) for a, b in zip(params[0], params[1])), 'plain run to run'
    assert torch.equal(losses[2], losses[0])
    assert all(torch.equal(a, b) for a, b in zip(params[2], params[0]))


def test_identity_second_pass_gives_the_constant(monkeypatch):
    """Identity st_cfg, mask_st=False, eval mode: the second pass sees the first pass's input bit for bit, its target is the
    first pass's flow bit for bit under the strict border mask, and its prediction is that flow up to what the model's forward
    itself gives at batch B and at batch 2B (the two directions stacked): max 1.1e-5, mean 2.4e-6 on an MI355X, with or without
    the vendor library held to its deterministic solvers (the step runs in the reproducible setting here).
    With d = |pred - flow_t| taken from the step's own call, the AR term must lie
        within the restatement's derived bound of loss(pred, flow_t, m), and
        between c (1 - 8 u) and (c + q eps^(q - 1) mean(d m) / (mean m + 1e-7)) (1 + 8 u)     ((d + eps)^q is concave in d),
    c = eps^q mean m / (mean m + 1e-7) the constant the formula gives at d = 0, sum m = B (H - 2) (W - 2); 8 u: powf within
    2 ulp, and eps, q as float32 numbers."""
    from arflow_amd.train_step import synthetic_pairs
    (B, (H, W)), eps, q = (2, STEP_HW), 0.01, 0.4
    x = synthetic_pairs(B, H, W, device=torch.device('cuda'), seed=5)
    seen = {}
    transform, loss = AR.ar_transform, AR.ar_loss

    def spy_transform(theta, img=None, flow=None, noc=None, **kw):
        out = transform(theta, img=img, flow=flow, noc=noc, **kw)
        seen.update(theta=theta, img=img, flow=flow, noc=noc, out=out)
        return out

    def spy_loss(pred, flow_t, mask=None, eps=0.0, q=1.0):
        seen.update(pred=pred.detach().clone(), flow_t=flow_t, mask=mask, eps=eps, q=q)
        return loss(pred, flow_t, mask, eps=eps, q=q)
    monkeypatch.setattr(AR, 'ar_transform', spy_transform)
    monkeypatch.setattr(AR, 'ar_loss', spy_loss)
    with reproducible():
        step = _step(dict(w_ar=0.01, ar_eps=eps, ar_q=q, mask_st=False, st_cfg={}))
        step.model.eval()
        step(x)
    img_t, flow_t, mask_t = seen['out']
    assert torch.equal(seen['theta'], AR.identity_theta(B)) and seen['noc'] is None and (seen['eps'], seen['q']) == (eps, q)
    assert torch.equal(seen['img'], x) and torch.equal(img_t, x) and torch.equal(flow_t, seen['flow']) and not flow_t.requires_grad
    assert torch.equal(mask_t, border((H, W)).expand(B, 1, H, W)) and seen['flow_t'] is flow_t and seen['mask'] is mask_t
    pred, m = seen['pred'].cpu(), mask_t.cpu()
    d = (pred - flow_t.cpu()).abs().double()
    mean_m = (H - 2) * (W - 2) / float(H * W)
    c = eps ** q * mean_m / (mean_m + 1e-7)
    upper = c + q * eps ** (q - 1) * float((d * m).sum() / (2 * B * H * W)) / (mean_m + 1e-7)
    want, _, e_want, _ = R.loss(pred, flow_t.cpu(), m, eps, q, track=True)
    got = float(step.last_ar)
    print('AR term %.9e, restated %.9e (bound %.3e), the constant %.9e, upper %.9e; passes differ by max %.3e mean %.3e'
          % (got, float(want), float(e_want), c, upper, float(d.max()), float(d.mean())))
    assert float(d.max()) <= 1e-4 * float(flow_t.abs().max())   # fp32 noise of two launch shapes, not another flow
    assert abs(got - float(want)) <= float(e_want)
    assert c * (1 - 8 * R.U) <= got <= upper * (1 + 8 * R.U)
    assert abs(got - c) <= (upper - c) + 8 * R.U * upper        # the gap to the constant is the passes' disagreement, no more
