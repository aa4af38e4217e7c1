"""GPU: the dilated context layers as phase mosaics on the split-bf16 kernels (csrc/phase.hip, csrc/phase_plan.hpp,
AF.DilatedChainFunction).

The layout is restated here in torch, one phase slice x[:, :, p::d, q::d] at a time (to_layout / from_layout), from the plan's
(Pg, Qg) alone; the kernels are compared with it bit for bit.

  1. phase_move: NCHW -> d -> NCHW is the identity bit for bit (full-mantissa values, signed zeros); d_a -> d_b equals going
     through NCHW; destinations pre-filled with NaN come back with exact zeros at every separator / tail and no NaN; a source
     whose separators hold NaN gives NaN-free output; the second destination holds the same values.
  2. forward and data gradient through the layout equal AF.splitconv (same transpose_flip, same epilogue) on every phase slice,
     bit for bit: the kernel forms the same sums in the same order.
  3. accuracy, measure e of tests/test_splitconv_gpu.py against float64 F.conv2d(padding=d, dilation=d) on the CPU: at most twice
     the library's e on the same GPU and inputs (the larger of two library runs) for y, dx and -- tests/test_splitconv_wgrad_gpu.py's
     criterion 1 -- dw.
  4. indexing is exact: a one-hot w gives the input shifted by ((r-1) d, (s-1) d) bit for bit over nine taps; a one-hot x gives
     dw[:, c, r, s] == dy[n, :, h - (r-1) d, w - (s-1) d] and exact zeros elsewhere, at the corners, on both sides of a separator
     and in a ragged last row / column.
  5. phase_act_bwd: gin is bit-equal to arflow_bias_act_bwd on the NCHW tensors moved afterwards; the bias gradient holds
     tests/test_hip_parity.py::test_bias_leaky_relu's bound against the float64 sum; NaN at the separators of gout and y reaches
     neither.
  6. the node at 2 x 128 x 21 x 37 against the composed ConvAct path on the same GPU within tests/test_dense_block_gpu.py's bound
     max(4 s, 1e-6 max|ref|), s = two composed runs' difference; two runs bitwise equal, also in deterministic mode; the model's
     state_dict keys unchanged; ContextNetwork reaches the node where the routing rule says so and not below the floor.

Shapes (N, C, K, H, W), each with d in {2, 4, 8, 16}: channel tails past a 16- and a 32-pad, K over gridDim.y, H % d and
W % d != 0, H == d (phases of one row).  H < d is refused before anything is launched.

Measured on MI355X (e in units of u = 2^-24; this tree / F.conv2d(dilation=d); also profiles/dilated_errors_vs_float64.log):
  2x40x33x21x37 d 2: y 4.884 / 20.574 u  dx 6.050 / 20.323 u  dw 1.384 / 9.640 u
  2x40x33x21x37 d 4: y 5.609 / 18.649 u  dx 6.416 / 16.904 u  dw 1.491 / 10.850 u
  2x40x33x21x37 d 8: y 4.572 / 18.894 u  dx 5.950 / 17.311 u  dw 1.373 / 10.474 u
  2x40x33x21x37 d 16: y 2.908 / 14.259 u  dx 3.514 / 12.482 u  dw 1.150 / 8.466 u
  1x17x70x16x33 d 2: y 3.340 / 13.559 u  dx 4.752 / 22.491 u  dw 1.683 / 4.352 u
  1x17x70x16x33 d 4: y 3.183 / 13.849 u  dx 3.776 / 24.757 u  dw 1.835 / 4.706 u
  1x17x70x16x33 d 8: y 2.005 / 9.418 u  dx 3.119 / 19.352 u  dw 1.695 / 4.310 u
  1x17x70x16x33 d 16: y 2.300 / 6.173 u  dx 2.740 / 12.104 u  dw 1.250 / 4.208 u
  2x128x96x19x32 d 2: y 4.140 / 10.064 u  dx 3.995 / 14.559 u  dw 1.473 / 5.499 u
  2x128x96x19x32 d 4: y 3.955 / 10.538 u  dx 4.238 / 16.372 u  dw 1.278 / 4.989 u
  2x128x96x19x32 d 8: y 3.468 / 9.623 u  dx 3.431 / 14.740 u  dw 1.432 / 5.499 u
  2x128x96x19x32 d 16: y 2.785 / 6.917 u  dx 2.632 / 9.539 u  dw 1.787 / 5.182 u
The node against the composed path at 2 x 128 x 21 x 37 (max |difference|, all three routings of the weight gradients): y 8.3e-7, d x 4.0e-7,
weights 9.5e-6 .. 2.6e-5, biases 6.7e-6 .. 9.5e-6, each inside max(4 s, 1e-6 max|ref|); the tightest is d convs.1.0.bias.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(2, 40, 33, 21, 37), (1, 17, 70, 16, 33), (2, 128, 96, 19, 32)]
DS = [2, 4, 8, 16]
CASES = [(s, d) for s in SHAPES for d in DS]
ids = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) and not isinstance(v[0], tuple) else '%s-d%d' % ('x'.join(map(str, v[0])), v[1])


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


# ---- the layout, restated --------------------------------------------------------------------------------------------
def cells(AF, N, H, W, d):
    """(phase p, phase q, virtual sample offset per real sample, first row, first column) of every cell."""
    Nv, Hv, Wv, Pg, Qg = AF.phase_layout(N, H, W, d)
    Hs, Ws = -(-H // d), -(-W // d)
    assert (Hv, Wv, Nv) == (Pg * (Hs + 1) - 1, Qg * (Ws + 1) - 1, N * d * d // (Pg * Qg))
    per = (d // Pg) * (d // Qg)
    return per, (Nv, Hv, Wv), [(p, q, (p // Pg) * (d // Qg) + q // Qg, (p % Pg) * (Hs + 1), (q % Qg) * (Ws + 1)) for p in range(d) for q in range(d)]


def to_layout(AF, x, d, fill=0.0):
    N, C, H, W = x.shape
    per, (Nv, Hv, Wv), cs = cells(AF, N, H, W, d)
    v = torch.full((N, per, C, Hv, Wv), fill, dtype=x.dtype, device=x.device)
    for p, q, g, r0, c0 in cs:
        cell = x[:, :, p::d, q::d]
        v[:, g, :, r0:r0 + cell.shape[2], c0:c0 + cell.shape[3]] = cell
    return v.view(Nv, C, Hv, Wv)


def from_layout(AF, v, N, H, W, d):
    per, (Nv, Hv, Wv), cs = cells(AF, N, H, W, d)
    C = v.shape[1]
    x = torch.empty(N, C, H, W, dtype=v.dtype, device=v.device)
    v = v.view(N, per, C, Hv, Wv)
    for p, q, g, r0, c0 in cs:
        cell = x[:, :, p::d, q::d]
        cell.copy_(v[:, g, :, r0:r0 + cell.shape[2], c0:c0 + cell.shape[3]])
    return x


def real_mask(AF, N, H, W, d):
    return to_layout(AF, torch.ones(N, 1, H, W, device='cuda'), d) > 0


def full_mantissa(*shape, seed):
    """Floats of either sign with all 24 significand bits random, over 14 binades."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 1 << 23, shape, generator=g) + (1 << 23)
    expo = torch.randint(-30, -16, shape, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g)
    return sign * torch.ldexp(bits.float(), expo)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. phase_move ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=ids)
def test_phase_move_is_the_layout_bit_for_bit(AF, case):
    (N, _, K, H, W), d = case
    x = full_mantissa(N, K, H, W, seed=d + H)
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = -0.0
    x = x.cuda()
    real = (N, H, W)
    ref = to_layout(AF, x, d)
    nan = lambda t: torch.full_like(t, float('nan'))
    v, plain = AF.phase_move(x, real, 1, d, 1, out=nan(ref), out2=nan(x))
    assert same_bits(v, ref), 'NCHW -> d differs from the slices (or a separator / tail is not an exact +0)'
    assert same_bits(plain, x), 'the second destination differs'
    back, _ = AF.phase_move(v, real, d, 1, out=nan(x))
    assert same_bits(back, x), 'NCHW -> d -> NCHW is not the identity'
    dirty = to_layout(AF, x, d, fill=float('nan'))  # what a convolution leaves: anything at separators and tails
    assert same_bits(AF.phase_move(dirty, real, d, 1)[0], x)
    for d2 in DS:
        if d2 <= min(H, W):
            ref2 = to_layout(AF, x, d2)
            got, also = AF.phase_move(dirty, real, d, d2, d, out=nan(ref2), out2=nan(ref))
            assert same_bits(got, ref2), 'd %d -> %d differs from going through NCHW' % (d, d2)
            assert same_bits(also, ref)


def test_a_map_smaller_than_the_dilation_is_refused_before_any_launch(AF):
    from arflow_amd import _lib
    x = torch.full((1, 3, 8, 40), 5.0, device='cuda')
    dst = torch.full((4096,), 7.0, device='cuda')
    with pytest.raises(_lib.ArflowHipError, match='-1002'):
        AF._call('arflow_phase_move', x.data_ptr(), dst.data_ptr(), None, 1, 3, 8, 40, 1, 16, 0, AF._stream())
    with pytest.raises(_lib.ArflowHipError, match='-1002'):
        AF._call('arflow_phase_act_bwd', x.data_ptr(), x.data_ptr(), dst.data_ptr(), None, None, 1, 3, 8, 40, 1, 16, 0, 0.1, AF._stream())
    with pytest.raises(_lib.ArflowHipError, match='-1002'):
        AF.phase_layout(1, 40, 8, 16)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((x == 5.0).all())


# ---- 2. the convolution through the layout is the convolution of every phase slice ---------------------------------------
@pytest.mark.parametrize('case', CASES, ids=ids)
def test_forward_and_data_gradient_equal_splitconv_on_every_phase_slice(AF, case):
    (N, C, K, H, W), d = case
    g = torch.Generator().manual_seed(C + d)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    gy = torch.randn(N, K, H, W, generator=g).cuda()
    w = torch.randn(K, C, 3, 3, generator=g).cuda()
    bias = torch.randn(K, generator=g).cuda()
    real = (N, H, W)
    y = AF.phase_move(AF.splitconv(AF.phase_move(x, real, 1, d)[0], w, bias=bias, slope=0.1), real, d, 1)[0]
    dx = AF.phase_move(AF.splitconv(AF.phase_move(gy, real, 1, d)[0], w, transpose_flip=True), real, d, 1)[0]
    for p in range(d):
        for q in range(d):
            ys = AF.splitconv(x[:, :, p::d, q::d].contiguous(), w, bias=bias, slope=0.1)
            assert torch.equal(y[:, :, p::d, q::d], ys), 'forward, phase (%d, %d)' % (p, q)
            ds = AF.splitconv(gy[:, :, p::d, q::d].contiguous(), w, transpose_flip=True)
            assert torch.equal(dx[:, :, p::d, q::d], ds), 'data gradient, phase (%d, %d)' % (p, q)


# ---- 3. accuracy against float64, and that the slices mean the dilated convolution ---------------------------------------
def inputs(N, C, K, H, W):
    g = torch.Generator().manual_seed(N * 1000003 + C * 10007 + K * 1009 + H * 131 + W)
    mk = lambda *s: 3.0 + torch.randn(*s, generator=g)
    return mk(N, C, H, W), mk(K, C, 3, 3), mk(N, K, H, W)


def conv64(x, w, gy, d):
    xs, ws = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xs, ws, None, 1, d, d)
    dx, dw = torch.autograd.grad(y, (xs, ws), gy.double())
    return y.detach(), dx, dw


def ratio(got, ref, s):
    err = (got.double().cpu() - ref).abs()
    return float(torch.where(s > 0, err / s.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0)).max())


def ours(AF, x, w, gy, d):
    N, _, H, W = x.shape
    real = (N, H, W)
    xv, gv = AF.phase_move(x, real, 1, d)[0], AF.phase_move(gy, real, 1, d)[0]
    y = AF.phase_move(AF.splitconv(xv, w), real, d, 1)[0]
    dx = AF.phase_move(AF.splitconv(gv, w, transpose_flip=True), real, d, 1)[0]
    return y, dx, AF.splitconv_wgrad(xv, gv)


def library(x, w, gy, d):
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xg, wg, None, 1, d, d)
    dx, dw = torch.autograd.grad(y, (xg, wg), gy)
    return y.detach(), dx, dw


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_dilated_conv_against_float64_and_the_library(AF, case):
    shape, d = case
    x, w, gy = inputs(*shape)
    ref = conv64(x, w, gy, d)
    S = conv64(x.abs(), w.abs(), gy.abs(), d)
    xg, wg, gg = x.cuda(), w.cuda(), gy.cuda()
    got, again = ours(AF, xg, wg, gg, d), ours(AF, xg, wg, gg, d)
    lib, lib2 = library(xg, wg, gg, d), library(xg, wg, gg, d)
    e_new = [ratio(g, r, s) for g, r, s in zip(got, ref, S)]
    e_lib = [max(ratio(a, r, s), ratio(b, r, s)) for a, b, r, s in zip(lib, lib2, ref, S)]
    print('dilated %s d %d: ' % (ids(shape), d) + '  '.join('%s %.3f / %.3f u' % (n, a / U, l / U) for n, a, l in zip(('y', 'dx', 'dw'), e_new, e_lib)))
    for n, a, c in zip(('y', 'dx', 'dw'), got, again):
        assert bool(torch.isfinite(a).all()), n
        assert torch.equal(a, c), '%s differs between two calls on the same inputs' % n
    for n, a, l in zip(('y', 'dx', 'dw'), e_new, e_lib):
        assert a <= 2.0 * l, '%s: e = %.3f u, more than twice the library\'s %.3f u' % (n, a / U, l / U)


# ---- 4. indexing ---------------------------------------------------------------------------------------------------------
def shifted(plane, dr, ds):
    """out[..., h, w] = plane[..., h + dr, w + ds], zero outside."""
    H, W = plane.shape[-2:]
    m = max(abs(dr), abs(ds))
    return F.pad(plane, (m, m, m, m))[..., m + dr:m + dr + H, m + ds:m + ds + W]


@pytest.mark.parametrize('case', [(SHAPES[0], d) for d in DS] + [(SHAPES[1], 16)], ids=ids)
def test_one_hot_weight_copies_the_shifted_plane_bit_for_bit(AF, case):
    (N, C, K, H, W), d = case
    x = full_mantissa(N, C, H, W, seed=17 * d).cuda()
    real = (N, H, W)
    xv = AF.phase_move(x, real, 1, d)[0]
    for tap, (k, c) in zip(range(9), [(0, 0), (K - 1, C - 1), (32 * ((K - 1) // 32), 16 * ((C - 1) // 16))] * 3):
        r, s = divmod(tap, 3)
        w = torch.zeros(K, C, 3, 3, device='cuda')
        w[k, c, r, s] = 1.0
        y = AF.phase_move(AF.splitconv(xv, w), real, d, 1)[0]
        assert torch.equal(y[:, k], shifted(x[:, c], (r - 1) * d, (s - 1) * d)), 'tap (%d, %d)' % (r, s)
        y[:, k] = 0
        assert not bool(y.any()), 'tap (%d, %d): another output channel is not exactly zero' % (r, s)


def hot_pixels(H, W, d):
    Hs, Ws = -(-H // d), -(-W // d)
    px = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}          # corners
    px |= {((H - 1) // d * d, (W - 1) // d * d), (1, 1)}           # last of phase 0's cell | first of phase 1's: a separator's two sides
    if Hs >= 2 and Ws >= 2:
        px |= {((Hs - 2) * d + d - 1, (Ws - 2) * d + d - 1)}        # last row / column of the last phase: ragged when d does not divide
    return sorted(p for p in px if p[0] < H and p[1] < W)


@pytest.mark.parametrize('case', [(SHAPES[0], d) for d in DS] + [(SHAPES[1], 16)], ids=ids)
def test_one_hot_input_copies_the_output_gradient_bit_for_bit(AF, case):
    (N, C, K, H, W), d = case
    gy = full_mantissa(N, K, H, W, seed=5 * d).cuda()
    real = (N, H, W)
    gv = AF.phase_move(gy, real, 1, d)[0]
    for i, (h, w) in enumerate(hot_pixels(H, W, d)):
        n, c = i % N, (C - 1, 0, 16 * ((C - 1) // 16))[i % 3]
        x = torch.zeros(N, C, H, W, device='cuda')
        x[n, c, h, w] = 1.0
        dw = AF.splitconv_wgrad(AF.phase_move(x, real, 1, d)[0], gv)
        ref = torch.zeros(K, C, 3, 3, device='cuda')
        for r in range(3):
            for s in range(3):
                hh, ww = h - (r - 1) * d, w - (s - 1) * d
                if 0 <= hh < H and 0 <= ww < W:
                    ref[:, c, r, s] = gy[n, :, hh, ww]
        assert torch.equal(dw, ref), 'pixel (%d, %d)' % (h, w)


# ---- 5. phase_act_bwd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=ids)
def test_act_bwd_equals_bias_act_bwd_moved_afterwards(AF, case):
    from tests.conftest import assert_close
    (N, _, K, H, W), d = case
    d_b = {2: 16, 4: 2, 8: 4, 16: 8}[d]
    if d_b > min(H, W):
        d_b = 1
    g = torch.Generator().manual_seed(d + W)
    gout = torch.randn(N, K, H, W, generator=g).cuda()
    y = torch.randn(N, K, H, W, generator=g).cuda()
    real = (N, H, W)
    ref = torch.empty_like(gout)
    AF._call('arflow_bias_act_bwd', gout.data_ptr(), y.data_ptr(), ref.data_ptr(), None, N, K, H * W, 0.1, AF._stream())
    exact = ref.double().sum((0, 2, 3))
    nan = float('nan')
    for d_a in (d, 1):
        gv, yv = (to_layout(AF, t, d_a, fill=nan) for t in (gout, y))
        gin, gin2, gb = AF.phase_act_bwd(gv, yv, real, d_a, d_b, 1, 0.1)
        assert same_bits(gin, to_layout(AF, ref, d_b)) and same_bits(gin2, ref), 'layout %d -> %d' % (d_a, d_b)
        assert_close(gb, exact, (1e-5 * max(1.0, float(exact.abs().max()))) / 2, 5e-6, 'gbias')
        again = AF.phase_act_bwd(gv, yv, real, d_a, d_b, 0, 0.1)
        assert same_bits(again[0], gin) and again[1] is None and torch.equal(again[2], gb)
        assert AF.phase_act_bwd(gv, yv, real, d_a, d_b, 0, 0.1, want_bias=False)[2] is None


# ---- 6. the node ---------------------------------------------------------------------------------------------------------
def _context(ch_in, seed):
    from arflow_amd.models import blocks
    torch.manual_seed(seed)
    net = blocks.ContextNetwork(ch_in)
    blocks.init_conv_weights(net, 'xavier')
    for p in net.parameters():  # non-zero biases, so that every term of the epilogue is exercised
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.05)
    return net.cuda()


def _chain(net, x, gy, node, AF):
    layers = net.convs[1:5]
    x = x.clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    if node:
        y = AF.dilated_chain(x, 0.1, [p for layer in layers for p in (layer[0].weight, layer[0].bias)])
    else:
        y = layers(x)
    y.backward(gy)
    return [y.detach(), x.grad] + [p.grad for layer in layers for p in (layer[0].weight, layer[0].bias)]


@pytest.mark.parametrize('wgrad', ['1111', '0000', None], ids=['native-dw', 'library-dw', 'routed-dw'])
def test_node_against_composed(AF, monkeypatch, wgrad):
    if wgrad is None:
        monkeypatch.delenv('ARFLOW_DILATED_WGRAD', raising=False)
    else:
        monkeypatch.setenv('ARFLOW_DILATED_WGRAD', wgrad)
    net = _context(40, 11)
    g = torch.Generator(device='cuda').manual_seed(7)
    x = torch.randn(2, 128, 21, 37, device='cuda', generator=g)
    gy = torch.randn(2, 64, 21, 37, device='cuda', generator=g)
    ref, ref2 = _chain(net, x, gy, False, AF), _chain(net, x, gy, False, AF)
    got, again = _chain(net, x, gy, True, AF), _chain(net, x, gy, True, AF)
    with AF.deterministic():
        det, det2 = _chain(net, x, gy, True, AF), _chain(net, x, gy, True, AF)
    names = ['y', 'd x'] + ['d convs.%d.0.%s' % (k, n) for k in range(1, 5) for n in ('weight', 'bias')]
    for n, a, b, c, e in zip(names, got, again, det, det2):
        if wgrad == '1111' or 'weight' not in n:  # MIOpen's weight gradient may end in atomics
            assert torch.equal(a, b), '%s differs between two runs' % n
            assert torch.equal(c, e) and torch.equal(a, c), '%s differs between two runs in deterministic mode' % n
    for n, a, r, r2 in zip(names, got, ref, ref2):
        s = float((r - r2).abs().max())
        err = float((a - r).abs().max())
        tol = max(4 * s, 1e-6 * float(r.abs().max()))
        print('%-24s |node - composed| %.3e   composed run to run %.3e   tol %.3e' % (n, err, s, tol))
        assert err <= tol, '%s: the node differs from composed by %.3e (two composed runs: %.3e, tol %.3e)' % (n, err, s, tol)


def test_context_network_routes_by_the_one_rule_and_keeps_its_keys(AF, monkeypatch):
    net = _context(40, 3)
    assert list(net.state_dict()) == ['convs.%d.0.%s' % (k, n) for k in range(7) for n in ('weight', 'bias')]
    x = torch.randn(2, 40, 21, 37, device='cuda')
    assert AF.dilated_chain_enabled() and not net.native(x)  # below the floor: the Sequential
    assert AF.dilated_chain_takes(16, 96, 160) and not AF.dilated_chain_takes(8, 96, 160) and not AF.dilated_chain_takes(16, 48, 80)
    calls = []
    real = AF.dilated_chain
    monkeypatch.setattr(AF, 'dilated_chain', lambda *a: (calls.append(1), real(*a))[1])
    ref = net(x)
    assert calls == []
    monkeypatch.setattr(AF, 'dilated_chain_takes', lambda N, H, W: True)
    assert net.native(x) and not net.native(x.cpu()) and not net.native(x.double())
    got = net(x)
    assert calls == [1]
    got.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert got.shape == ref.shape  # the values are test_node_against_composed's business
    monkeypatch.undo()
    monkeypatch.setattr(AF, '_DILATED_CHAIN', False)
    assert not AF.dilated_chain_takes(16, 96, 160)
