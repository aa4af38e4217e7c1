"""GPU: the wide 3x3 convolution on the bf16 matrix cores at fp32 accuracy (csrc/splitconv.hip behind
arflow_amd.functional.conv3x3, both halves forced onto the kernel) against a float64 F.conv2d on the CPU and against
F.conv2d and its autograd on the same GPU.

Measure (that of tests/test_headconv_gpu.py):  e = max over elements of |err| / S,  err = difference from the float64 result,
S = the same operation applied to absolute values in float64.  Inputs have mean 3, std 1, so no cancellation flatters the
error, and border rows and columns are compared like any others.

  1. forward and data gradient: e is at most TWICE the e of F.conv2d and its autograd on the same GPU and inputs;
  2. two calls give bitwise-equal y and dx;
  3. indexing is exact: with a one-hot w (a single 1.0 at (k, c, r, s)) and full-mantissa random x, y[k] is the shifted x[c]
     bit for bit and every other output channel is exactly zero -- every partial sum of the three bf16 planes of a float is
     representable, so any order is exact -- over all nine taps, the first and the last real channel and a channel of the
     last, partly padded tile; likewise the data gradient; and again with a one-hot x and random w;
  4. the weight gradient AF.conv3x3 returns equals F.conv2d's autograd's within max(4 s, 1e-6 max|ref|), s being what two
     calls of the latter differ by (tests/test_dense_block_gpu.py's bound).

Shapes (N, C, K, H, W): the smallest at which each mechanism can fail -- a single pixel; C and K just past a 16- and a 32-pad;
three channel tiles with W crossing the 32-pixel tile and H crossing 8 (the 16 x 2 pixel tile); the coarsest flagship layer;
rows long enough for several 32 x 1 tiles; the data-gradient orientation with K over gridDim.y in chunks of 2 and 1 tiles;
and a narrow, tall map (the 8 x 4 pixel tile).

Measured on MI355X (e in units of u = 2^-24; kernel / F.conv2d; also profiles/splitconv_errors_vs_float64.log):
  1x1x1x1x1: y 0.251 / 0.251 u  dx 0.060 / 0.060 u  dw |diff| 0 (MIOpen moves 0, max|dw| 8)
  2x3x2x5x7: y 1.234 / 0.855 u  dx 1.208 / 0.918 u  dw |diff| 0 (MIOpen moves 0, max|dw| 705)
  1x17x33x13x21: y 2.917 / 7.822 u  dx 5.195 / 9.416 u  dw |diff| 0 (MIOpen moves 0, max|dw| 2.63e+03)
  3x40x96x9x35: y 5.278 / 14.570 u  dx 4.427 / 14.996 u  dw |diff| 0.00293 (MIOpen moves 0.00293, max|dw| 8.99e+03)
  2x147x128x12x20: y 3.758 / 23.595 u  dx 4.209 / 5.517 u  dw |diff| 0 (MIOpen moves 0, max|dw| 4.69e+03)
  1x160x32x33x130: y 3.901 / 19.301 u  dx 6.872 / 10.515 u  dw |diff| 0.0117 (MIOpen moves 0.0117, max|dw| 3.97e+04)
  2x32x147x12x20: y 5.927 / 14.314 u  dx 3.550 / 23.100 u  dw |diff| 0.000977 (MIOpen moves 0.000977, max|dw| 4.74e+03)
  1x33x40x20x8: y 5.062 / 12.748 u  dx 3.976 / 10.139 u  dw |diff| 0 (MIOpen moves 0, max|dw| 1.63e+03)

MIOpen's own e moves between runs where its solver ends in atomics (dx at 1x17x33x13x21: 3.3 u in one run, 9.4 u in another).
At 2x3x2x5x7 it is correctly rounded (a solver with double accumulators), which is the tightest case for criterion 1.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 5, 7), (1, 17, 33, 13, 21), (3, 40, 96, 9, 35), (2, 147, 128, 12, 20), (1, 160, 32, 33, 130),
          (2, 32, 147, 12, 20), (1, 33, 40, 20, 8)]
ids = lambda s: 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


def inputs(N, C, K, H, W):
    g = torch.Generator().manual_seed(N * 1000003 + C * 10007 + K * 1009 + H * 131 + W)
    mk = lambda *s: 3.0 + torch.randn(*s, generator=g)
    return mk(N, C, H, W), mk(K, C, 3, 3), mk(N, K, H, W)


def conv64(x, w, gy):
    """float64 F.conv2d on the CPU and its data gradient for the upstream gy."""
    xs = x.double().requires_grad_(True)
    y = F.conv2d(xs, w.double(), None, 1, 1)
    dx, = torch.autograd.grad(y, xs, gy.double())
    return y.detach(), dx


def ratio(got, ref, s):
    return float(((got.double() - ref).abs() / s).max())


def gpu_grads(fn, x, w, gy):
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = fn(xg, wg)
    dx, dw = torch.autograd.grad(y, (xg, wg), gy.cuda())
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, dx, dw)]


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_conv3x3_against_float64_and_miopen(AF, shape):
    x, w, gy = inputs(*shape)
    ref = conv64(x, w, gy)
    S = conv64(x.abs(), w.abs(), gy.abs())
    got = gpu_grads(AF.conv3x3, x, w, gy)
    again = gpu_grads(AF.conv3x3, x, w, gy)
    lib = gpu_grads(lambda a, k: F.conv2d(a, k, None, 1, 1), x, w, gy)
    lib2 = gpu_grads(lambda a, k: F.conv2d(a, k, None, 1, 1), x, w, gy)
    e_new = [ratio(g, r, s) for g, r, s in zip(got, ref, S)]
    e_lib = [ratio(g, r, s) for g, r, s in zip(lib, ref, S)]
    move = float((lib[2] - lib2[2]).abs().max())
    dw_err = float((got[2] - lib[2]).abs().max())
    print('splitconv %s: ' % ids(shape) + '  '.join('%s %.3f / %.3f u' % (n, a / U, l / U) for n, a, l in zip(('y', 'dx'), e_new, e_lib)) +
          '  dw |diff| %.3g (MIOpen moves %.3g, max|dw| %.3g)' % (dw_err, move, float(lib[2].abs().max())))
    for n, a, c in zip(('y', 'dx'), got, again):
        assert torch.equal(a, c), '%s differs between two calls on the same inputs' % n
    for n, g in zip(('y', 'dx', 'dw'), got):
        assert bool(torch.isfinite(g).all()), n
    for n, a, l in zip(('y', 'dx'), e_new, e_lib):
        assert a <= 2.0 * l, '%s: e = %.3f u, more than twice F.conv2d\'s %.3f u' % (n, a / U, l / U)
    assert dw_err <= max(4 * move, 1e-6 * float(lib[2].abs().max()))


def full_mantissa(*shape, seed):
    """Floats of either sign with all 24 significand bits random, over 14 binades."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 1 << 23, shape, generator=g) + (1 << 23)
    expo = torch.randint(-30, -16, shape, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g)
    return sign * torch.ldexp(bits.float(), expo)


def shifted(plane, dr, ds):
    """out[..., h, w] = plane[..., h + dr, w + ds], zero outside."""
    H, W = plane.shape[-2:]
    return F.pad(plane, (1, 1, 1, 1))[..., 1 + dr:1 + dr + H, 1 + ds:1 + ds + W]


@pytest.mark.parametrize('shape', [(1, 17, 33, 13, 21), (2, 32, 147, 12, 20)], ids=ids)
def test_one_hot_weight_copies_the_shifted_plane_bit_for_bit(AF, shape):
    N, C, K, H, W = shape
    x = full_mantissa(N, C, H, W, seed=1).cuda()
    gy = full_mantissa(N, K, H, W, seed=2).cuda()
    picks = [(0, 0), (K - 1, C - 1), (32 * ((K - 1) // 32), 16 * ((C - 1) // 16))]  # first, last, first of the last (padded) tile
    for k, c in picks:
        for tap in range(9):
            r, s = divmod(tap, 3)
            w = torch.zeros(K, C, 3, 3, device='cuda')
            w[k, c, r, s] = 1.0
            xg = x.clone().requires_grad_(True)
            y = AF.conv3x3(xg, w)
            dx, = torch.autograd.grad(y, xg, gy)
            want_y = torch.zeros_like(y)
            want_y[:, k] = shifted(x[:, c], r - 1, s - 1)
            want_dx = torch.zeros_like(x)
            want_dx[:, c] = shifted(gy[:, k], 1 - r, 1 - s)
            assert torch.equal(y, want_y), (k, c, r, s)
            assert torch.equal(dx, want_dx), (k, c, r, s)


@pytest.mark.parametrize('shape', [(1, 17, 33, 13, 21), (2, 32, 147, 12, 20), (1, 33, 40, 20, 8)], ids=ids)
def test_one_hot_input_copies_the_weights_bit_for_bit(AF, shape):
    N, C, K, H, W = shape
    w = full_mantissa(K, C, 3, 3, seed=3).cuda()
    for n, c, h, q in [(0, 0, 0, 0), (N - 1, C - 1, H - 1, W - 1), (0, 16 * ((C - 1) // 16), H // 2, W // 2), (N - 1, C // 2, 7, W - 1)]:
        x = torch.zeros(N, C, H, W, device='cuda')
        x[n, c, h, q] = 1.0
        y = AF.conv3x3(x, w)
        want = torch.zeros_like(y)
        for r in range(3):
            for s in range(3):  # y[n, k, h - (r - 1), q - (s - 1)] = w[k, c, r, s]
                hh, qq = h - (r - 1), q - (s - 1)
                if 0 <= hh < H and 0 <= qq < W:
                    want[n, :, hh, qq] = w[:, c, r, s]
        assert torch.equal(y, want), (n, c, h, q)
        gy = torch.zeros(N, K, H, W, device='cuda')  # the data gradient: one-hot gy at (n, k, h, q)
        k = min(K - 1, c)
        gy[n, k, h, q] = 1.0
        xg = torch.zeros(N, C, H, W, device='cuda', requires_grad=True)
        dx, = torch.autograd.grad(AF.conv3x3(xg, w), xg, gy)
        want = torch.zeros_like(dx)
        for r in range(3):
            for s in range(3):  # dx[n, c, h + (r - 1), q + (s - 1)] = w[k, c, r, s]
                hh, qq = h + (r - 1), q + (s - 1)
                if 0 <= hh < H and 0 <= qq < W:
                    want[n, :, hh, qq] = w[k, :, r, s]
        assert torch.equal(dx, want), (n, k, h, q)


def test_needs_input_grad_is_honoured_and_halves_can_stay_on_miopen(AF):
    x, w, gy = inputs(2, 20, 40, 9, 12)
    full = gpu_grads(AF.conv3x3, x, w, gy)
    for want in ((True, False), (False, True)):
        ts = [t.cuda().requires_grad_(r) for t, r in zip((x, w), want)]
        g, = torch.autograd.grad(AF.conv3x3(*ts), [t for t, r in zip(ts, want) if r], gy.cuda())
        assert torch.equal(g.cpu(), full[1 if want[0] else 2])
    lib = gpu_grads(lambda a, k: F.conv2d(a, k, None, 1, 1), x, w, gy)
    only_fwd = gpu_grads(lambda a, k: AF.conv3x3(a, k, True, False), x, w, gy)
    only_dgrad = gpu_grads(lambda a, k: AF.conv3x3(a, k, False, True), x, w, gy)
    assert torch.equal(only_fwd[0], full[0]) and torch.equal(only_fwd[1], lib[1])
    assert torch.equal(only_dgrad[0], lib[0]) and torch.equal(only_dgrad[1], full[1])


def test_modules_route_by_the_one_predicate(AF, monkeypatch):
    """ConvAct and the fused dense estimator ask AF.splitconv_takes for the same layer and so run the same kernel: with every
    shape routed, fused and composed agree bit for bit, and the split kernel is what ran."""
    from arflow_amd.models import blocks
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(AF, '_splitconv_rule', lambda *a: True)
    calls = []
    real = AF.splitconv
    monkeypatch.setattr(AF, 'splitconv', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(0)
    est = blocks.FlowEstimatorDense(19).cuda()
    x = torch.randn(2, 19, 10, 12, device='cuda')
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(AF, '_DENSE_BLOCK', fused)
        calls.clear()
        xg = x.clone().requires_grad_(True)
        x6, flow = est(xg)
        gx, = torch.autograd.grad(x6.sum() + (flow * flow).sum(), xg)
        assert len(calls) == 10  # five forwards, five data gradients
        out[fused] = (x6.detach(), flow.detach(), gx)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert float((out[True][2] - out[False][2]).abs().max()) <= 1e-5 * float(out[False][2].abs().max())
    monkeypatch.setattr(AF, '_SPLITCONV', False)  # the switch restores the vendor path
    calls.clear()
    est(x)
    assert calls == []
    monkeypatch.setattr(AF, '_SPLITCONV', True)
    monkeypatch.setattr(blocks, 'bias_act', lambda t, bias, s: t)  # a twin that swaps bias_act out keeps F.conv2d
    assert est.conv1.split_route(x) == (False, False)
