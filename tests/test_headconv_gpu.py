"""GPU: the direct two-channel 3x3 head convolution (csrc/headconv.hip behind arflow_amd.functional.head_conv) against a
float64 F.conv2d on the CPU, all three passes, at the five head shapes of the flagship and at shapes that miss every
tile and chunk boundary.

Measure, per pass:  e = max over elements of |err| / S,  err = difference from the float64 result, S = the same
operation applied to absolute values in float64 (forward: conv(|x|, |w|) + |bias|; likewise the gradients; dbias
against dy.sum with S = |dy|.sum).  Inputs have mean 3, std 1, so no cancellation flatters the error, and border rows and
columns are compared like any others.

  1. The kernel's e must not exceed TWICE the e of F.conv2d and its autograd on the same GPU and inputs (what the
     layers ran before).  The factor two covers the run-to-run movement of the vendor library's atomic split-K weight
     gradient and the fact that a different summation order is not a worse one.
  2. Forward and data gradient: every element within n u / (1 - n u) * S, u = 2^-24, n = 9 C + 1 (forward) or 18 (data
     gradient) -- the bound of ANY fp32 summation order; it catches a dropped tap, channel or border.
  3. Two calls on the same inputs give bitwise-equal y, dx, dw, dbias.

Measured on MI355X (e in units of u = 2^-24; kernel / F.conv2d):
(y, dx, dw, dbias; also profiles/headconv_errors_vs_float64.log)
  1x1x1x1: y 0.144 / 0.144 u  dx 0.487 / 0.487 u  dw 0.790 / 0.790 u  dbias 0.000 / 0.000 u
  3x1x1x1: y 0.621 / 0.621 u  dx 0.453 / 0.453 u  dw 0.410 / 0.410 u  dbias 0.610 / 0.610 u
  1x1x5x7: y 0.863 / 1.292 u  dx 0.647 / 0.647 u  dw 0.815 / 0.815 u  dbias 0.285 / 0.285 u
  3x1x5x7: y 0.928 / 1.524 u  dx 0.953 / 0.953 u  dw 0.703 / 1.919 u  dbias 0.516 / 1.265 u
  1x1x13x21: y 0.928 / 1.472 u  dx 0.956 / 3.585 u  dw 0.967 / 1.013 u  dbias 0.500 / 0.500 u
  3x1x13x21: y 0.945 / 1.475 u  dx 0.889 / 4.768 u  dw 0.639 / 3.526 u  dbias 0.797 / 0.797 u
  1x1x33x130: y 0.971 / 5.576 u  dx 0.982 / 5.047 u  dw 0.774 / 5.164 u  dbias 0.415 / 0.855 u
  3x1x33x130: y 0.980 / 8.257 u  dx 0.979 / 5.344 u  dw 0.535 / 8.427 u  dbias 0.705 / 0.705 u
  1x3x1x1: y 0.685 / 0.717 u  dx 0.829 / 0.829 u  dw 0.910 / 0.910 u  dbias 0.000 / 0.000 u
  3x3x1x1: y 0.838 / 1.159 u  dx 0.814 / 0.814 u  dw 0.851 / 0.851 u  dbias 0.384 / 0.384 u
  1x3x5x7: y 0.878 / 1.696 u  dx 0.959 / 0.959 u  dw 0.795 / 0.795 u  dbias 0.212 / 0.212 u
  3x3x5x7: y 0.861 / 1.573 u  dx 0.951 / 0.951 u  dw 0.815 / 3.760 u  dbias 0.800 / 0.800 u
  1x3x13x21: y 0.954 / 1.816 u  dx 0.882 / 4.046 u  dw 0.927 / 10.229 u  dbias 0.309 / 0.945 u
  3x3x13x21: y 0.978 / 1.651 u  dx 0.961 / 4.638 u  dw 0.628 / 4.199 u  dbias 0.154 / 1.624 u
  1x3x33x130: y 0.994 / 4.237 u  dx 0.996 / 5.959 u  dw 0.865 / 8.734 u  dbias 0.288 / 0.997 u
  3x3x33x130: y 0.998 / 5.405 u  dx 0.995 / 7.150 u  dw 0.547 / 12.840 u  dbias 0.560 / 0.560 u
  1x97x1x1: y 0.513 / 0.513 u  dx 0.929 / 0.929 u  dw 0.961 / 0.961 u  dbias 0.000 / 0.000 u
  3x97x1x1: y 0.567 / 8.349 u  dx 0.951 / 0.951 u  dw 0.933 / 0.933 u  dbias 0.952 / 0.952 u
  1x97x5x7: y 0.778 / 3.843 u  dx 0.978 / 0.978 u  dw 0.983 / 4.200 u  dbias 0.424 / 0.424 u
  3x97x5x7: y 0.773 / 12.384 u  dx 0.994 / 0.994 u  dw 0.864 / 5.391 u  dbias 0.747 / 0.916 u
  1x97x13x21: y 0.781 / 5.951 u  dx 0.994 / 6.273 u  dw 0.980 / 4.518 u  dbias 0.540 / 0.540 u
  3x97x13x21: y 0.790 / 11.321 u  dx 0.993 / 8.629 u  dw 0.639 / 5.531 u  dbias 0.554 / 1.843 u
  1x97x33x130: y 0.944 / 11.166 u  dx 0.997 / 6.826 u  dw 0.884 / 7.433 u  dbias 0.549 / 0.721 u
  3x97x33x130: y 0.804 / 12.152 u  dx 0.999 / 8.837 u  dw 0.587 / 7.300 u  dbias 0.294 / 0.294 u
  2x5x13x20: y 0.963 / 4.558 u  dx 0.980 / 5.022 u  dw 0.946 / 3.794 u  dbias 0.394 / 0.394 u
  1x19x7x12: y 0.979 / 4.216 u  dx 0.976 / 0.976 u  dw 0.957 / 4.310 u  dbias 0.518 / 0.935 u
  3x2x1x4: y 0.827 / 1.262 u  dx 0.797 / 0.797 u  dw 0.789 / 0.789 u  dbias 0.131 / 0.131 u
  2x40x6x8: y 0.967 / 10.227 u  dx 0.996 / 0.996 u  dw 0.842 / 5.610 u  dbias 0.603 / 0.603 u
  16x595x96x160: y 0.974 / 36.687 u  dx 1.000 / 10.448 u  dw 0.965 / 41.520 u  dbias 0.657 / 0.657 u
  16x595x48x80: y 0.991 / 44.087 u  dx 1.000 / 10.693 u  dw 0.982 / 20.098 u  dbias 0.406 / 0.406 u
  16x595x24x40: y 0.933 / 42.251 u  dx 0.999 / 11.090 u  dw 0.994 / 11.123 u  dbias 0.449 / 1.168 u
  16x563x12x20: y 0.805 / 51.531 u  dx 0.998 / 10.948 u  dw 0.995 / 11.131 u  dbias 0.591 / 0.834 u
  16x32x96x160: y 0.880 / 10.338 u  dx 1.000 / 8.173 u  dw 0.960 / 9.101 u  dbias 0.100 / 0.100 u
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLAGSHIP = [(16, 595, 96, 160), (16, 595, 48, 80), (16, 595, 24, 40), (16, 563, 12, 20), (16, 32, 96, 160)]
AWKWARD = [(B, C, H, W) for C in (1, 3, 97) for (H, W) in ((1, 1), (5, 7), (13, 21), (33, 130)) for B in (1, 3)]
# W % 4 == 0 (the float4 path) with rows that do not fill the last strip, a last wave that is not full, C below one slice
ALIGNED_TAILS = [(2, 5, 13, 20), (1, 19, 7, 12), (3, 2, 1, 4), (2, 40, 6, 8)]


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


def inputs(B, C, H, W):
    g = torch.Generator().manual_seed(B * 1000003 + C * 10007 + H * 131 + W)
    mk = lambda *s: 3.0 + torch.randn(*s, generator=g)
    return mk(B, C, H, W), mk(2, C, 3, 3), mk(2), mk(B, 2, H, W)


def conv64(x, w, b, dy, chunk=2):
    """float64 F.conv2d on the CPU and its gradients for the upstream dy; samples in chunks to bound the memory."""
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ys, dxs = [], []
    dw, db = torch.zeros_like(w64), torch.zeros_like(b64)
    for i in range(0, x.shape[0], chunk):
        xs = x[i:i + chunk].double().requires_grad_(True)
        y = F.conv2d(xs, w64, b64, 1, 1)
        gx, gw, gb = torch.autograd.grad(y, (xs, w64, b64), dy[i:i + chunk].double())
        ys.append(y.detach()), dxs.append(gx)
        dw += gw
        db += gb
    return torch.cat(ys), torch.cat(dxs), dw, db


def ratio(got, ref, s, scale=1.0):
    """max |err| / (scale * S); where S is zero (a tap that only ever meets the zero padding) the result must be exact."""
    err = (got.double() - ref).abs()
    inf = torch.full_like(err, float('inf'))
    return float(torch.where(s > 0, err / (scale * s).clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err))).max())


def gpu_grads(fn, x, w, b, dy):
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = fn(xg, wg, bg)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.cuda())
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, dx, dw, db)]


@pytest.mark.parametrize('shape', FLAGSHIP + AWKWARD + ALIGNED_TAILS, ids=lambda s: 'x'.join(map(str, s)))
def test_head_conv_against_float64(AF, shape):
    B, C, H, W = shape
    x, w, b, dy = inputs(B, C, H, W)
    ref = conv64(x, w, b, dy)
    S = conv64(x.abs(), w.abs(), b.abs(), dy.abs())
    got = gpu_grads(AF.head_conv, x, w, b, dy)
    again = gpu_grads(AF.head_conv, x, w, b, dy)
    lib = gpu_grads(lambda a, k, c: F.conv2d(a, k, c, 1, 1), x, w, b, dy)
    names = ['y', 'dx', 'dw', 'dbias']
    e_new = [ratio(g, r, s) for g, r, s in zip(got, ref, S)]
    e_lib = [ratio(g, r, s) for g, r, s in zip(lib, ref, S)]
    print('headconv %s: ' % 'x'.join(map(str, shape)) +
          '  '.join('%s %.3f / %.3f u' % (n, a / U, l / U) for n, a, l in zip(names, e_new, e_lib)))
    for n, a, c in zip(names, got, again):
        assert torch.equal(a, c), '%s differs between two calls on the same inputs' % n
    for n, g in zip(names, got):
        assert bool(torch.isfinite(g).all()), n
    for n_terms, k in ((9 * C + 1, 0), (18, 1)):
        gamma = n_terms * U / (1 - n_terms * U)
        worst = ratio(got[k], ref[k], S[k], gamma)
        assert worst <= 1.0, '%s: |err| is %.3f of the fp32 summation bound (n = %d)' % (names[k], worst, n_terms)
    for n, a, l in zip(names, e_new, e_lib):
        assert a <= 2.0 * l, '%s: e = %.3f u, more than twice F.conv2d\'s %.3f u' % (n, a / U, l / U)


def test_head_conv_needs_input_grad_subsets(AF):
    """Only the gradients autograd asks for are computed, and each equals the full call's bit for bit."""
    x, w, b, dy = inputs(2, 7, 9, 12)
    full = gpu_grads(AF.head_conv, x, w, b, dy)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        ts = [t.cuda().requires_grad_(r) for t, r in zip((x, w, b), want)]
        y = AF.head_conv(*ts)
        grads = torch.autograd.grad(y, [t for t, r in zip(ts, want) if r], dy.cuda())
        expect = [f for f, r in zip(full[1:], want) if r]
        for gq, ex in zip(grads, expect):
            assert torch.equal(gq.cpu(), ex)
    y = AF.head_conv(x.cuda(), w.cuda(), None)  # no bias
    assert torch.equal(y.cpu(), gpu_grads(lambda a, k, c: AF.head_conv(a, k, c * 0), x, w, b, dy)[0])


def test_flow_head_module_takes_the_native_path(AF, monkeypatch):
    from arflow_amd.models import blocks
    head = blocks.conv(8, 2, isReLU=False).cuda()
    x = torch.randn(2, 8, 10, 12, device='cuda')
    calls = []
    real = AF.head_conv
    monkeypatch.setattr(AF, 'head_conv', lambda *a: (calls.append(1), real(*a))[1])
    y = head(x)
    assert calls == [1]
    ref = F.conv2d(x, head[0].weight, head[0].bias, 1, 1)
    assert float((y - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6
    monkeypatch.setattr(blocks, 'bias_act', lambda t, bias, s: t)  # a twin that swaps bias_act out keeps F.conv2d
    head(x)
    assert calls == [1]
