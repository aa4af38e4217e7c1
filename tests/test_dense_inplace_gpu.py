"""GPU: the dense flow estimator in place -- arflow_splitconv_fwd_ex reading a channel slice and
writing bias + LeakyReLU into a channel slot of the same tensor, and AF.DenseEstimatorFunction built on it -- against the
path it replaces (splitconv into a fresh tensor, then arflow_dense_cat_fwd).

  1. AF.splitconv(x_view, w, out=slot, bias=b, slope=s) is AF.bias_leaky_relu(AF.splitconv(x_view.contiguous(), w), b, s), bit
     for bit, and leaves every element outside the slot untouched;
  2. input and output as disjoint channel ranges of ONE buffer give the bits separate tensors give;
  3. the estimator with _DENSE_INPLACE on and off: x6, flow, the input and bias gradients bit for bit; the weight gradients
     bit for bit where both come from splitconv_wgrad, else within max(4 * s, 1e-6 * max|ref|), s = two runs of the parent's
     path (the bound of tests/test_dense_block_gpu.py);
  4. partial gradients, as tests/test_dense_block_gpu.py::test_estimator_partial_gradients_and_no_grad, on the in-place path.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FILL = 0x7FC12345  # a NaN with a payload: no kernel produces it, and int32 comparison sees every bit


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    return functional


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _filled(*shape):
    return torch.full(shape, FILL, device='cuda', dtype=torch.int32).view(torch.float32)


# (N, C, K, H, W, transpose_flip)
EX_SHAPES = [
    (2, 19, 70, 10, 12, False),   # channel tail; K in two chunks of KT 2 + 1; narrow pixel tile
    (1, 40, 96, 9, 35, False),    # KT 2 + 1; 32-wide tile with a column tail
    (3, 33, 32, 20, 8, False),    # KT 1; 8 x 4 tile; C one past a block
    (2, 64, 147, 13, 21, True),   # five output tiles in three chunks of KT 2, 2, 1; the data-gradient form
]


@pytest.mark.parametrize('shape', EX_SHAPES, ids=lambda s: 'x'.join(str(int(v)) for v in s))
def test_slice_in_slot_out_epilogue_equals_the_composed_call(AF, shape):
    N, C, K, H, W, tf = shape
    g = _gen(3)
    big = torch.randn(N, C + 5, H, W, device='cuda', generator=g)
    xv = big[:, 5:]  # the channel suffix of a larger tensor
    w = 0.1 * torch.randn(*((C, K) if tf else (K, C)), 3, 3, device='cuda', generator=g)
    b = torch.randn(K, device='cuda', generator=g)
    plain = AF.splitconv(xv.contiguous(), w, transpose_flip=tf)
    assert torch.equal(AF.splitconv(xv, w, transpose_flip=tf), plain)  # the slice read in place
    for bias, slope in ((b, 0.1), (None, 0.1), (None, None)):
        ref = plain if slope is None else AF.bias_leaky_relu(plain.clone(), bias, slope)
        outer = _filled(N, K + 7, H, W)
        slot = outer[:, 3:3 + K]
        got = AF.splitconv(xv, w, transpose_flip=tf, out=slot, bias=bias, slope=slope)
        assert got is slot
        assert torch.equal(slot, ref), (bias is not None, slope)
        keep = outer.view(torch.int32)
        assert bool((keep[:, :3] == FILL).all()) and bool((keep[:, 3 + K:] == FILL).all())
    with pytest.raises(ValueError):
        AF.splitconv(xv, w, transpose_flip=tf, bias=b)  # a bias needs the epilogue
    with pytest.raises(ValueError):
        AF.splitconv(xv, w, transpose_flip=tf, out=torch.empty(N, K, W, H, device='cuda').transpose(2, 3))


def test_input_and_output_in_one_buffer(AF):
    N, C, K, H, W = 2, 19, 70, 10, 12
    g = _gen(4)
    x = torch.randn(N, C, H, W, device='cuda', generator=g)
    w = 0.1 * torch.randn(K, C, 3, 3, device='cuda', generator=g)
    b = torch.randn(K, device='cuda', generator=g)
    ref = AF.splitconv(x, w, out=torch.empty(N, K, H, W, device='cuda'), bias=b, slope=0.1)
    buf = _filled(N, K + C, H, W)
    buf[:, K:].copy_(x)
    AF.splitconv(buf[:, K:], w, out=buf[:, :K], bias=b, slope=0.1)
    assert torch.equal(buf[:, :K], ref) and torch.equal(buf[:, K:], x)
    with pytest.raises(ValueError):
        AF.splitconv(buf[:, K:], w, out=buf[:, 1:K + 1], bias=b, slope=0.1)  # the slot reaches into the input


def _estimator(ch_in, seed):  # tests/test_dense_block_gpu.py::_estimator
    from arflow_amd.models import blocks
    torch.manual_seed(seed)
    est = blocks.FlowEstimatorDense(ch_in)
    blocks.init_conv_weights(est, 'xavier')
    for p in est.parameters():  # non-zero biases, so that every term of the epilogue is exercised
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.05)
    return est.cuda()


def _count(AF, monkeypatch, name, calls):
    real = getattr(AF, name)
    monkeypatch.setattr(AF, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])


def _run(est, x, gx6, gflow, inplace, monkeypatch, AF):
    monkeypatch.setattr(AF, '_DENSE_INPLACE', inplace)
    x = x.clone().requires_grad_(True)
    est.zero_grad(set_to_none=True)
    x6, flow = est(x)
    saved = len(x6.grad_fn.saved_tensors)
    assert x6.is_contiguous()
    torch.autograd.backward([x6, flow], [gx6, gflow])
    return [x6.detach(), flow.detach(), x.grad] + [p.grad for p in est.parameters()], saved


@pytest.mark.parametrize('wgrad_ours', [False, True], ids=['dw-miopen', 'dw-splitconv'])
@pytest.mark.parametrize('shape', [(2, 19, 10, 12), (3, 33, 9, 20)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_estimator_in_place_against_the_parents_path(AF, monkeypatch, shape, wgrad_ours):
    B, C, H, W = shape
    assert AF.dense_block_enabled() and AF.splitconv_enabled()
    est = _estimator(C, 11)
    g = _gen(7)
    x = torch.randn(B, C, H, W, device='cuda', generator=g)
    gx6 = torch.randn(B, C + 448, H, W, device='cuda', generator=g)
    gflow = torch.randn(B, 2, H, W, device='cuda', generator=g)
    calls = []
    _count(AF, monkeypatch, 'dense_cat', calls)
    _count(AF, monkeypatch, 'splitconv', calls)
    # the real rule keeps these small shapes on the parent's path, switch on or off
    _, saved = _run(est, x, gx6, gflow, True, monkeypatch, AF)
    assert calls.count('dense_cat') == 5 and calls.count('splitconv') == 0 and saved == 12
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: True)
    if wgrad_ours:
        monkeypatch.setattr(AF, '_SPLITCONV_WGRAD', True)
        monkeypatch.setattr(AF, '_splitconv_wgrad_rule', lambda *a: True)
    calls.clear()
    ref, saved_ref = _run(est, x, gx6, gflow, False, monkeypatch, AF)
    assert calls.count('dense_cat') == 5 and calls.count('splitconv') == 10 and saved_ref == 12
    ref2, _ = _run(est, x, gx6, gflow, False, monkeypatch, AF)
    calls.clear()
    got, saved = _run(est, x, gx6, gflow, True, monkeypatch, AF)
    assert calls.count('dense_cat') == 0 and calls.count('splitconv') == 10 and saved < 12
    assert torch.equal(got[0], ref[0]), 'x6'
    assert torch.equal(got[1], ref[1]), 'flow'
    assert torch.equal(got[2], ref[2]), 'the input gradient'  # all five data gradients are on the deterministic kernel
    names = [n for n, _ in est.named_parameters()]
    for n, a, r, r2 in zip(names, got[3:], ref[3:], ref2[3:]):
        s = float((r - r2).abs().max())
        err = float((a - r).abs().max())
        tol = max(4 * s, 1e-6 * float(r.abs().max()))
        print('%-24s |in place - parent| %.3e   parent run to run %.3e   tol %.3e' % (n, err, s, tol))
        if n.endswith('bias') or wgrad_ours or n.startswith('conv_last'):
            assert torch.equal(a, r), n  # the gather's fixed-order fold; splitconv_wgrad; the head's own kernels
        else:
            assert err <= tol, '%s: in place differs from the parent by %.3e (two parent runs: %.3e, tol %.3e)' % (n, err, s, tol)


def test_estimator_in_place_partial_gradients_and_no_grad(AF, monkeypatch):
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: True)
    monkeypatch.setattr(AF, '_DENSE_INPLACE', True)
    calls = []
    _count(AF, monkeypatch, 'dense_cat', calls)
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
    assert x6.is_contiguous() and not calls  # every pass above ran in place
