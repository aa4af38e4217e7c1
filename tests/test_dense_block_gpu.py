"""GPU: the dense flow estimator's two kernels (csrc/dense.hip) and the autograd node built on them
(AF.DenseEstimatorFunction) against the composed path they replace.

  1. arflow_dense_cat_fwd is torch.cat([bias_leaky_relu(y, b, s), x], 1), bit for bit;
  2. arflow_dense_grad_gather is the sum of its sources in the documented nesting followed by arflow_bias_act_bwd: gy bit for
     bit, the bias gradient within the bound tests/test_hip_parity.py::test_bias_leaky_relu uses (here against the float64 sum
     of the reference gy) and bit-identical between two calls;
  3. the whole estimator, fused against composed in one process: outputs bit for bit, gradients within
     max(4 * s, 1e-6 * max|ref|) where s is what two runs of the COMPOSED path differ by (MIOpen's split-K weight gradients use
     atomics; the factor 4 leaves room for a third draw of the same noise).
"""
import pytest
import torch

from tests.conftest import assert_close

pytestmark = pytest.mark.gpu

LAYERS = [(147, 128), (275, 128), (403, 96), (499, 64), (563, 32)]  # (C, oc) of the five layers at the finest level


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


CAT_SHAPES = ([(4, oc, C, h, w, 0.1) for h, w in ((12, 20), (24, 40)) for C, oc in LAYERS] + [(16, 32, 563, 96, 160, 0.1)] +
              [(1, 1, 3, 5, 7, 1.0), (3, 5, 2, 3, 3, 0.1), (1, 1, 1, 1, 1, 0.1), (2, 3, 4, 67, 63, 0.25), (2, 7, 1, 2, 6, 1.0)])


@pytest.mark.parametrize('shape', CAT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_cat_fwd_equals_bias_act_then_cat(AF, shape):
    B, oc, C, H, W, slope = shape
    g = _gen(3)
    y = torch.randn(B, oc, H, W, device='cuda', generator=g)
    x = torch.randn(B, C, H, W, device='cuda', generator=g)
    b = torch.randn(oc, device='cuda', generator=g)
    ref = torch.cat([AF.bias_leaky_relu(y.clone(), b, slope), x], 1)
    got = AF.dense_cat(y, b, x, slope)
    assert got.shape == ref.shape and got.is_contiguous()
    assert torch.equal(got, ref)
    assert torch.equal(AF.dense_cat(y, None, x, slope), torch.cat([AF.bias_leaky_relu(y.clone(), None, slope), x], 1))


def _composed_gather(AF, sources, oc, act, slope):
    """The tensor expression in the documented nesting, then arflow_bias_act_bwd (direct C call: gin, gbias)."""
    from arflow_amd import _lib
    acc = None
    for t, off, scale in sources:
        s = t[:, off:off + oc]
        if scale is not None:
            s = s * scale.view(-1, 1, 1, 1)
        acc = s if acc is None else s + acc
    acc = acc.contiguous()
    if act is None:
        return acc, None
    B, _, H, W = acc.shape
    y = act[:, :oc].contiguous()
    gin, gb = torch.empty_like(acc), torch.empty(oc, device='cuda')
    rc = _lib.load().arflow_bias_act_bwd(acc.data_ptr(), y.data_ptr(), gin.data_ptr(), gb.data_ptr(), B, oc, H * W, slope,
                                         torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'arflow_bias_act_bwd')
    return gin, gb


# (B, oc, H, W, channels of every source tensor, slope, index of the scaled source or None, with activation)
GATHER_CASES = [
    (4, 32, 12, 20, [595], 0.1, None, True),                                 # 1 source
    (4, 32, 24, 40, [595, 595], 0.1, 0, True),                               # 2: x6's gradient (scaled) + the head's
    (4, 128, 12, 20, [595, 595, 563, 499, 403, 275], 0.1, None, True),       # layer 1's activation: 6 sources
    (2, 147, 24, 40, [595, 595, 563, 499, 403, 275, 147], 0.1, 0, False),    # d/dx1: 7 sources, no activation, scaled
    (16, 64, 96, 160, [595, 595, 563], 0.1, None, True),                     # layer 4 at the finest level of the flagship
    (3, 5, 3, 3, [9, 6], 0.25, 1, True),                                     # HW % 4 != 0
    (1, 1, 5, 7, [1, 4, 2, 3, 1, 1, 1, 2], 1.0, None, True),                 # 8 sources, B = 1, oc = 1, slope 1
    (2, 3, 67, 63, [4, 3], 0.1, 0, False),                                   # ragged, several chunks per plane
]


@pytest.mark.parametrize('case', GATHER_CASES, ids=lambda c: '%dx%dx%dx%d-%dsrc' % (c[0], c[1], c[2], c[3], len(c[4])))
def test_grad_gather_equals_nested_sum_then_bias_act_bwd(AF, case):
    B, oc, H, W, chans, slope, scaled, with_act = case
    g = _gen(5)
    sources = []
    for j, c in enumerate(chans):
        t = torch.randn(B, c, H, W, device='cuda', generator=g)
        scale = None
        if j == scaled:
            scale = torch.ones(B, device='cuda')
            scale[B // 2] = 0.0  # a dropped sample
        sources.append((t, c - oc if j % 2 == 0 else 0, scale))  # slices at the end and at the start of their tensors
    act = torch.randn(B, oc + 3, H, W, device='cuda', generator=g) if with_act else None
    ref_gy, ref_gb = _composed_gather(AF, sources, oc, act, slope)
    gy, gb = AF.dense_grad_gather(sources, oc, act=act, slope=slope, want_bias=with_act)
    assert gy.is_contiguous() and torch.equal(gy, ref_gy)
    if scaled is not None and with_act is False:
        assert float(ref_gy[B // 2].abs().max()) > 0  # only the scaled source is dropped there
    if with_act:
        exact = ref_gy.double().sum((0, 2, 3))
        print('gbias: max |err| vs float64 %.3e (fused) %.3e (bias_act_bwd), max |gbias| %.3e'
              % (float((gb - exact).abs().max()), float((ref_gb - exact).abs().max()), float(exact.abs().max())))
        assert_close(gb, exact, (1e-5 * max(1.0, float(exact.abs().max()))) / 2, 5e-6, 'gbias')
        again = AF.dense_grad_gather(sources, oc, act=act, slope=slope, want_bias=True)[1]
        assert torch.equal(gb, again)  # fixed-order fold
        assert AF.dense_grad_gather(sources, oc, act=act, slope=slope)[1] is None
    else:
        assert gb is None


def _estimator(ch_in, seed):
    from arflow_amd.models import blocks
    torch.manual_seed(seed)
    est = blocks.FlowEstimatorDense(ch_in)
    blocks.init_conv_weights(est, 'xavier')
    for p in est.parameters():  # non-zero biases, so that every term of the epilogue is exercised
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.05)
    return est.cuda()


def _run(est, x, gx6, gflow, fused, monkeypatch, AF):
    monkeypatch.setattr(AF, '_DENSE_BLOCK', fused)
    calls = []
    real = AF.dense_estimator
    monkeypatch.setattr(AF, 'dense_estimator', lambda *a: (calls.append(1), real(*a))[1])
    x = x.clone().requires_grad_(True)
    est.zero_grad(set_to_none=True)
    x6, flow = est(x)
    monkeypatch.setattr(AF, 'dense_estimator', real)
    assert calls == ([1] if fused else [])
    torch.autograd.backward([x6, flow], [gx6, gflow])
    return [x6.detach(), flow.detach(), x.grad] + [p.grad for p in est.parameters()]


@pytest.mark.parametrize('shape', [(4, 147, 24, 40), (16, 115, 12, 20)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_estimator_fused_against_composed(AF, monkeypatch, shape):
    B, C, H, W = shape
    est = _estimator(C, 11)
    g = _gen(7)
    x = torch.randn(B, C, H, W, device='cuda', generator=g)
    gx6 = torch.randn(B, C + 448, H, W, device='cuda', generator=g)
    gflow = torch.randn(B, 2, H, W, device='cuda', generator=g)
    ref = _run(est, x, gx6, gflow, False, monkeypatch, AF)
    ref2 = _run(est, x, gx6, gflow, False, monkeypatch, AF)
    got = _run(est, x, gx6, gflow, True, monkeypatch, AF)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    names = ['d x1'] + ['d ' + n for n, _ in est.named_parameters()]
    for n, a, r, r2 in zip(names, got[2:], ref[2:], ref2[2:]):
        s = float((r - r2).abs().max())
        err = float((a - r).abs().max())
        tol = max(4 * s, 1e-6 * float(r.abs().max()))
        print('%-24s |fused - composed| %.3e   composed run to run %.3e   tol %.3e' % (n, err, s, tol))
        assert err <= tol, '%s: fused differs from composed by %.3e (two composed runs: %.3e, tol %.3e)' % (n, err, s, tol)


def test_estimator_partial_gradients_and_no_grad(AF):
    assert AF.dense_block_enabled()
    est = _estimator(19, 13)
    g = _gen(9)
    x = torch.randn(2, 19, 12, 20, device='cuda', generator=g)
    # the input needs no gradient
    est.zero_grad(set_to_none=True)
    x6, flow = est(x)
    (x6.square().mean() + flow.square().mean()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in est.parameters())
    full = {n: p.grad.clone() for n, p in est.named_parameters()}
    # only one of the two outputs is used
    xr = x.clone().requires_grad_(True)
    est.zero_grad(set_to_none=True)
    est(xr)[1].square().mean().backward()
    assert xr.grad is not None and all(p.grad is not None for p in est.parameters())
    xr = x.clone().requires_grad_(True)
    est.zero_grad(set_to_none=True)
    est(xr)[0].square().mean().backward()
    assert xr.grad is not None and est.conv_last[0].weight.grad is None and est.conv1[0].weight.grad is not None
    # frozen weights: the lower layers, then everything but the input
    est.zero_grad(set_to_none=True)
    for layer in (est.conv1, est.conv2, est.conv3):
        for p in layer.parameters():
            p.requires_grad_(False)
    x6, flow = est(x)
    (x6.square().mean() + flow.square().mean()).backward()
    assert est.conv1[0].weight.grad is None and est.conv3[0].bias.grad is None
    for n in ('conv4.0.weight', 'conv5.0.bias', 'conv_last.0.weight'):
        got, ref = dict(est.named_parameters())[n].grad, full[n]
        assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-7, n  # same values as the unfrozen run
    for p in est.parameters():
        p.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    x6, flow = est(xr)
    (x6.square().mean() + flow.square().mean()).backward()
    assert xr.grad is not None and bool(torch.isfinite(xr.grad).all())
    with torch.no_grad():
        x6, flow = est(x)
    assert not x6.requires_grad and x6.shape == (2, 19 + 448, 12, 20) and flow.shape == (2, 2, 12, 20)


def test_models_reach_the_fused_node(AF, monkeypatch):
    """PWCLiteUflow (the flagship) gets the node through the module at every level."""
    from arflow_amd.config import AttrDict
    from arflow_amd.train_step import WORKLOADS
    from arflow_amd.models import get_model
    calls = []
    real = AF.dense_estimator
    monkeypatch.setattr(AF, 'dense_estimator', lambda *a: (calls.append(tuple(a[0].shape)), real(*a))[1])
    torch.manual_seed(0)
    model = get_model(AttrDict(WORKLOADS['pwclite_uflow+uflow_loss'][0])).cuda()
    model.init_weights()
    model.train()
    img = torch.rand(1, 6, 256, 384, device='cuda')
    out = model(img, with_bk=True)
    assert len(calls) == 4 and all(c[0] == 2 for c in calls)
    sum(f.square().mean() for f in out['flows_fw'] + out['flows_bw']).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
