"""GPU: the routing of the weight gradients to csrc/splitconv_wgrad.hip.  With the rule forced to always-true the dense flow
estimator as ONE autograd node (AF.dense_estimator) and as the composed ConvAct chain run the same kernel on the same values
for the same layer: their parameter gradients are torch.equal (the kernel is deterministic, which MIOpen's weight gradients are
not).  With ARFLOW_SPLITCONV_WGRAD off, or the weight frozen, nothing is launched; the unpatched rule refuses every shape
below N H W = 16 x 48 x 80."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def _estimator(ch_in, seed):
    from arflow_amd.models import blocks
    torch.manual_seed(seed)
    est = blocks.FlowEstimatorDense(ch_in)
    blocks.init_conv_weights(est, 'xavier')
    for p in est.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.05)
    return est.cuda()


def _run(est, x, gx6, gflow, fused, monkeypatch, AF):
    monkeypatch.setattr(AF, '_DENSE_BLOCK', fused)
    calls = []
    real = AF.splitconv_wgrad
    monkeypatch.setattr(AF, 'splitconv_wgrad', lambda a, b: (calls.append((a.shape[1], b.shape[1])), real(a, b))[1])
    x = x.clone().requires_grad_(True)
    est.zero_grad(set_to_none=True)
    x6, flow = est(x)
    torch.autograd.backward([x6, flow], [gx6, gflow])
    torch.cuda.synchronize()
    monkeypatch.setattr(AF, 'splitconv_wgrad', real)
    return calls, [x6.detach(), flow.detach(), x.grad] + [p.grad for p in est.parameters()]


def _case(C=19, B=2, H=12, W=20, seed=3):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, C, H, W, device='cuda', generator=g)
    gx6 = torch.randn(B, C + 448, H, W, device='cuda', generator=g)
    gflow = torch.randn(B, 2, H, W, device='cuda', generator=g)
    return x, gx6, gflow


def test_fused_and_composed_run_the_same_kernel(AF, monkeypatch):
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    monkeypatch.setattr(AF, '_splitconv_wgrad_rule', lambda *a: True)
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: True)  # forward and data gradient deterministic as well
    est = _estimator(19, 11)
    x, gx6, gflow = _case()
    layers = [(19, 128), (147, 128), (275, 96), (371, 64), (435, 32)]  # (C, K) of conv1 .. conv5
    c_calls, composed = _run(est, x, gx6, gflow, False, monkeypatch, AF)
    f_calls, fused = _run(est, x, gx6, gflow, True, monkeypatch, AF)
    assert sorted(c_calls) == layers and sorted(f_calls) == layers  # the new function is what ran, once per layer
    for name, a, b in zip(['x6', 'flow', 'd x'] + [n for n, _ in est.named_parameters()], fused, composed):
        assert torch.equal(a, b), name  # same kernels on the same values, all of them deterministic
    # and it IS the weight gradient: MIOpen's, with the path off, agrees to fp32 accumulation error (both are within a few
    # tens of u of sum |terms|, which for these zero-mean operands is about ten times max |dw|)
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', False)
    off_calls, off = _run(est, x, gx6, gflow, True, monkeypatch, AF)
    assert off_calls == []
    for (name, _), a, b in zip(est.named_parameters(), fused[3:], off[3:]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), name


def test_switch_off_and_frozen_weight_launch_nothing(AF, monkeypatch):
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_splitconv_wgrad_rule', lambda *a: True)
    est = _estimator(19, 12)
    x, gx6, gflow = _case(seed=4)
    for fused in (False, True):
        monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', False)
        assert _run(est, x, gx6, gflow, fused, monkeypatch, AF)[0] == []
        monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
        est.conv2[0].weight.requires_grad_(False)  # needs_input_grad: no launch for the frozen 147 -> 128 weight
        calls, grads = _run(est, x, gx6, gflow, fused, monkeypatch, AF)
        est.conv2[0].weight.requires_grad_(True)
        assert sorted(calls) == [(19, 128), (275, 96), (371, 64), (435, 32)]
        assert est.conv2[0].weight.grad is None and est.conv2[0].bias.grad is not None and grads[2] is not None


def test_unpatched_rule_refuses_below_the_floor(AF, monkeypatch):
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
    for N, H, W in ((16, 24, 40), (8, 48, 80), (16, 48, 79), (4, 96, 160), (2, 12, 20)):
        for C, K in ((147, 128), (275, 128), (403, 96), (499, 64), (563, 32), (597, 128), (64, 32)):
            assert not AF.splitconv_wgrad_takes(N, C, K, H, W)
    est = _estimator(19, 13)
    x, gx6, gflow = _case(seed=5)
    for fused in (False, True):  # and so a small map keeps MIOpen's weight gradients
        assert _run(est, x, gx6, gflow, fused, monkeypatch, AF)[0] == []
