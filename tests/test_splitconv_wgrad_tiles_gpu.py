"""GPU: the 2 x 2 tiling of the split-bf16 weight gradient (csrc/splitconv_wgrad.hip): a workgroup owns
KT <= 2 tiles of 32 output channels times CT <= 2 tiles of 32 input channels, the input-channel parts are decoded from the
block id behind the XCD remap.  AF.splitconv_wgrad is called directly, so the routing floor does not matter.  Reference,
error measure e = |err| / sum |a b| and inputs are those of tests/test_splitconv_wgrad_gpu.py, imported from it.

Shapes (N, C, K, H, W), small ones at which the tiling can still go wrong:
  input-channel pairs and tails
    1x33x32x5x9     a pair whose second tile holds one channel; W odd: scalar staging loads, <KT 1, CT 2>
    1x65x33x6x16    a pair plus a single tile in one launch (the single tile's second half of the workgroup idles), KT = 2
    2x97x65x4x24    two pairs, the second one channel past its first tile; output-channel chunks of 2 and 1 tiles
    1x64x64x3x8     exactly one 2 x 2 workgroup
    1x65x40x5x9     scalar staging loads at KT = 2: that launch keeps single input-channel tiles (three of them)
  strip and row-block edges with CT = 2
    1x40x40x9x72    two strips of 6 and 3 groups
    1x33x33x40x16   one unit, so ten row blocks of MIN_ROWS = 4
    1x34x35x130x8   33 row blocks, the last of two rows (so small a shape never reaches MAX_ROWS rows per chunk: that
                    bound is walked on the host, tests/test_splitconv_wgrad_plan_cpu.py)
Criteria: those of the existing test -- e at most twice aten.convolution_backward's (the larger of two runs), two calls bitwise
equal; a one-hot operand reproduces the other bit for bit; a channel slice of a larger tensor gives the packed call's bits.
"""
import pytest
import torch

from tests import test_splitconv_wgrad_gpu as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 33, 32, 5, 9), (1, 65, 33, 6, 16), (2, 97, 65, 4, 24), (1, 64, 64, 3, 8), (1, 65, 40, 5, 9), (1, 40, 40, 9, 72),
          (1, 33, 33, 40, 16), (1, 34, 35, 130, 8)]


@pytest.fixture(scope='module')
def AF():
    from arflow_amd import functional
    torch.set_num_threads(16)
    return functional


@pytest.mark.parametrize('shape', SHAPES, ids=T.ids)
def test_tiles_against_float64_and_miopen(AF, shape):
    x, gy = T.inputs(*shape)
    ref, S = T.dw64(x, gy), T.dw64(x.abs(), gy.abs())
    xg, gyg = x.cuda(), gy.cuda()
    got, again = AF.splitconv_wgrad(xg, gyg), AF.splitconv_wgrad(xg, gyg)
    e_new = T.ratio(got, ref, S)
    e_lib = max(T.ratio(T.lib_dw(xg, gyg), ref, S), T.ratio(T.lib_dw(xg, gyg), ref, S))
    print('splitconv_wgrad tiles %s: dw %.3f / %.3f u' % (T.ids(shape), e_new / T.U, e_lib / T.U))
    assert tuple(got.shape) == (shape[2], shape[1], 3, 3) and bool(torch.isfinite(got).all())
    assert torch.equal(got, again), 'dw differs between two calls on the same inputs'
    assert e_new <= 2.0 * e_lib, 'dw: e = %.3f u, more than twice aten.convolution_backward\'s %.3f u' % (e_new / T.U, e_lib / T.U)


# (N, C, K, H, W) = (1, 80, 80, 11, 72): C tiles 32 + 32 + 16 as a pair and a single tile, K tiles the same as chunks of 2 and 1;
# 9 groups of 8 columns in strips of 6 and 3 (boundary at column 48); 8 units, so row blocks of 4 (boundaries at rows 4 and 8)
ONE_HOT = (1, 80, 80, 11, 72)
PIXELS = [(0, 0), (0, 71), (10, 0), (10, 71), (3, 47), (4, 48), (7, 40), (8, 55)]
CHANNELS = (31, 32, 64, 79)  # last of the pair's first tile, first of its second, first and last of the trailing single tile


@pytest.mark.parametrize('hot', ['x', 'dy'])
def test_one_hot_in_a_pair_reproduces_the_other_operand_bit_for_bit(AF, hot):
    N, C, K, H, W = ONE_HOT
    other = T.full_mantissa(N, K if hot == 'x' else C, H, W, seed=15 if hot == 'x' else 16)
    og = other.cuda()
    nch = C if hot == 'x' else K
    for h, w in PIXELS:
        for ch in CHANNELS:
            one = torch.zeros(N, nch, H, W)
            one[0, ch, h, w] = 1.0
            dw = (AF.splitconv_wgrad(one.cuda(), og) if hot == 'x' else AF.splitconv_wgrad(og, one.cuda())).cpu()
            want = torch.zeros(K, C, 3, 3)
            for r in range(3):
                for s in range(3):
                    if hot == 'x':  # dw[:, c, r, s] = dy[n, :, h - (r - 1), w - (s - 1)]
                        hh, ww = h - (r - 1), w - (s - 1)
                        if 0 <= hh < H and 0 <= ww < W:
                            want[:, ch, r, s] = other[0, :, hh, ww]
                    else:  # dw[k, :, r, s] = x[n, :, h + r - 1, w + s - 1]
                        want[ch, :, r, s] = T.shifted(other[0], r - 1, s - 1)[:, h, w]
            assert torch.equal(dw, want), 'one-hot %s at channel %d pixel (%d, %d)' % (hot, ch, h, w)


@pytest.mark.parametrize('shape', [(2, 65, 40, 6, 16), (2, 97, 65, 4, 24)], ids=T.ids)
def test_channel_slice_across_a_pair_boundary_is_read_in_place(AF, shape):
    N, C, K, H, W = shape
    x, gy = T.inputs(*shape)
    xbig = torch.randn(N, C + 5, H, W).cuda()
    gbig = torch.randn(N, K + 3, H, W).cuda()
    xbig[:, 3:3 + C] = x.cuda()
    gbig[:, 2:2 + K] = gy.cuda()
    xs, gs = xbig[:, 3:3 + C], gbig[:, 2:2 + K]
    assert not xs.is_contiguous() and xs.stride(0) == (C + 5) * H * W
    packed = AF.splitconv_wgrad(x.cuda(), gy.cuda())
    assert torch.equal(AF.splitconv_wgrad(xs, gs), packed)
    assert torch.equal(AF.splitconv_wgrad(xs, gy.cuda()), packed) and torch.equal(AF.splitconv_wgrad(x.cuda(), gs), packed)
