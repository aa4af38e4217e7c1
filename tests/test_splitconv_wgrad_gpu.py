"""GPU: the weight gradient of the wide 3x3 convolution on the bf16 matrix cores at fp32 accuracy (csrc/splitconv_wgrad.hip,
called directly through arflow_amd.functional.splitconv_wgrad, so the routing rule does not matter) against the float64 weight
gradient on the CPU and against aten.convolution_backward on the same GPU.

Measure (that of tests/test_splitconv_gpu.py):  e = max over elements of |dw - dw64| / S,  dw64 the float64 weight gradient,
S the same operation applied to absolute values.  Inputs are 3 + randn, so no cancellation flatters the error.

  1. accuracy: e is at most TWICE the e of aten.convolution_backward (mask [False, True, False]) on the same GPU and inputs,
     the library's larger e of two runs (its result moves where the solver ends in atomics);
  2. two calls give bitwise-equal dw;
  3. indexing is exact: with a one-hot x (a single 1.0 at (n, c, h, w)) and full-mantissa dy,
     dw[:, c, r, s] == dy[n, :, h - (r - 1), w - (s - 1)] bit for bit where that pixel exists and everything else is exactly
     zero -- every partial sum of the three bf16 planes of a float is representable, so any order is exact; a one-hot dy gives
     the symmetric statement.  Pixels: the four corners, the last row, the last column, both sides of a strip boundary and of a
     row-block boundary (the pixel chunks); channels: the first and the last real one and the first of the last, partly padded
     tile of C and of K;
  4. x and dy passed as channel slices of larger tensors (batch stride larger than C H W) give the packed call's bits.

Shapes (N, C, K, H, W): a single pixel; W < 8 and odd; C and K just past a 16- and a 32-pad with W no multiple of 8; three K
tiles (chunks of 2 and 1) with W past 32; the coarsest flagship layer; a narrow, tall map; and a long reduction with narrow
channels: 61 440 terms in 384 pixel chunks folded by the finish kernel.

Measured on MI355X (e in u = 2^-24; kernel / aten.convolution_backward, the larger of two runs; also
profiles/splitconv_wgrad_errors_vs_float64.log):
  1x1x1x1x1: dw 1.253 / 0.629 u
  2x3x2x5x7: dw 1.402 / 0.865 u
  1x17x33x13x21: dw 2.234 / 14.979 u
  3x40x96x9x35: dw 1.717 / 5.537 u
  2x147x128x12x20: dw 1.917 / 9.721 u
  1x33x40x20x8: dw 1.840 / 12.338 u
  16x32x32x48x80: dw 1.069 / 10.814 u

At 1x1x1x1x1 and 2x3x2x5x7 MIOpen is correctly rounded (a solver with double accumulators); these are the tightest cases for
criterion 1.  A single product carries the three dropped plane products (below 2.01 u of it) and nothing averages them: 1.253 u
against the bound of 1.258 u.  MIOpen's e moves between runs where its solver ends in atomics (1x17x33x13x21: 4.6 u in one
job, 15.0 u in another).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 5, 7), (1, 17, 33, 13, 21), (3, 40, 96, 9, 35), (2, 147, 128, 12, 20), (1, 33, 40, 20, 8),
          (16, 32, 32, 48, 80)]
ids = lambda s: 'x'.join(map(str, s))
CONV_ARGS = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


def inputs(N, C, K, H, W):
    g = torch.Generator().manual_seed(N * 1000003 + C * 10007 + K * 1009 + H * 131 + W)
    return 3.0 + torch.randn(N, C, H, W, generator=g), 3.0 + torch.randn(N, K, H, W, generator=g)


def dw64(x, gy):
    """The float64 weight gradient of conv2d(x, w, padding=1) on the CPU."""
    w = torch.zeros(gy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x.double(), w, None, 1, 1), w, gy.double())[0]


def lib_dw(xg, gyg):
    w = torch.empty(gyg.shape[1], xg.shape[1], 3, 3, device='cuda')
    return torch.ops.aten.convolution_backward(gyg, xg, w, None, *CONV_ARGS, [False, True, False])[1]


def ratio(got, ref, s):
    """max |err| / S; where S == 0 (a tap that meets no pixel: a one-row or one-column map) the element must be exactly 0."""
    err = (got.double().cpu() - ref).abs()
    return float(torch.where(s > 0, err / s.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0)).max())


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_wgrad_against_float64_and_miopen(AF, shape):
    x, gy = inputs(*shape)
    ref, S = dw64(x, gy), dw64(x.abs(), gy.abs())
    xg, gyg = x.cuda(), gy.cuda()
    got, again = AF.splitconv_wgrad(xg, gyg), AF.splitconv_wgrad(xg, gyg)
    e_new = ratio(got, ref, S)
    e_lib = max(ratio(lib_dw(xg, gyg), ref, S), ratio(lib_dw(xg, gyg), ref, S))
    print('splitconv_wgrad %s: dw %.3f / %.3f u' % (ids(shape), e_new / U, e_lib / U))
    assert tuple(got.shape) == (shape[2], shape[1], 3, 3) and bool(torch.isfinite(got).all())
    assert torch.equal(got, again), 'dw differs between two calls on the same inputs'
    assert e_new <= 2.0 * e_lib, 'dw: e = %.3f u, more than twice aten.convolution_backward\'s %.3f u' % (e_new / U, e_lib / U)


def full_mantissa(*shape, seed):
    """Floats of either sign with all 24 significand bits random, over 14 binades."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 1 << 23, shape, generator=g) + (1 << 23)
    expo = torch.randint(-30, -16, shape, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g)
    return sign * torch.ldexp(bits.float(), expo)


# (N, C, K, H, W) = (2, 40, 70, 11, 75): 10 groups of 8 columns in strips of 6 and 4 (boundary at column 48), row blocks of 4
# (boundaries at rows 4 and 8); C tiles 32 + 8, K tiles 32 + 32 + 6 in chunks of 2 and 1
ONE_HOT = (2, 40, 70, 11, 75)
PIXELS = [(0, 0), (0, 74), (10, 0), (10, 74), (10, 37), (5, 74), (3, 47), (4, 48), (7, 40), (8, 55)]


def shifted(plane, dr, ds):
    """out[..., h, w] = plane[..., h + dr, w + ds], zero outside."""
    H, W = plane.shape[-2:]
    return F.pad(plane, (1, 1, 1, 1))[..., 1 + dr:1 + dr + H, 1 + ds:1 + ds + W]


@pytest.mark.parametrize('hot', ['x', 'dy'])
def test_one_hot_operand_reproduces_the_other_bit_for_bit(AF, hot):
    N, C, K, H, W = ONE_HOT
    other = full_mantissa(N, K if hot == 'x' else C, H, W, seed=5 if hot == 'x' else 6)
    og = other.cuda()
    nch = C if hot == 'x' else K
    for j, (h, w) in enumerate(PIXELS):
        for ch in (0, nch - 1, 32 * ((nch - 1) // 32)):
            n = j % N
            one = torch.zeros(N, nch, H, W)
            one[n, ch, h, w] = 1.0
            dw = (AF.splitconv_wgrad(one.cuda(), og) if hot == 'x' else AF.splitconv_wgrad(og, one.cuda())).cpu()
            want = torch.zeros(K, C, 3, 3)
            for r in range(3):
                for s in range(3):
                    if hot == 'x':  # dw[:, c, r, s] = dy[n, :, h - (r - 1), w - (s - 1)]
                        hh, ww = h - (r - 1), w - (s - 1)
                        if 0 <= hh < H and 0 <= ww < W:
                            want[:, ch, r, s] = other[n, :, hh, ww]
                    else:  # dw[k, :, r, s] = x[n, :, h + r - 1, w + s - 1]
                        want[ch, :, r, s] = shifted(other[n], r - 1, s - 1)[:, h, w]
            assert torch.equal(dw, want), 'one-hot %s at n %d channel %d pixel (%d, %d)' % (hot, n, ch, h, w)


@pytest.mark.parametrize('shape', [(2, 3, 2, 5, 7), (3, 40, 96, 9, 35)], ids=ids)
def test_channel_slices_of_larger_tensors_are_read_in_place(AF, shape):
    N, C, K, H, W = shape
    x, gy = inputs(*shape)
    xbig = torch.randn(N, C + 5, H, W).cuda()
    gbig = torch.randn(N, K + 3, H, W).cuda()
    xbig[:, 3:3 + C] = x.cuda()
    gbig[:, 2:2 + K] = gy.cuda()
    xs, gs = xbig[:, 3:3 + C], gbig[:, 2:2 + K]
    assert not xs.is_contiguous() and xs.stride(0) == (C + 5) * H * W
    packed = AF.splitconv_wgrad(x.cuda(), gy.cuda())
    assert torch.equal(AF.splitconv_wgrad(xs, gs), packed)
    assert torch.equal(AF.splitconv_wgrad(xs, gy.cuda()), packed) and torch.equal(AF.splitconv_wgrad(x.cuda(), gs), packed)
